"""Cases and the derived bound for the GMM statistics tests (csrc/kh_gmmacc.hip, tests/gmm_acc_restatement.py).

THE BOUND.  An output element (a Gaussian's occ, mean_acc[d] or var_acc[d]) is the sum over the n entries of its pdf of
addends t_e = p_e, p_e x_e or p_e x_e^2, p and x floats widened to double.  p x is exact in double (48 bits), x^2 too, p x^2
rounds once.  Whatever the order of the n - 1 additions (the library: per chunk of CHUNK entries in frame order by fused
multiply-adds, the chunks in chunk order; the restatement: frame by frame), each rounds once, relative to a partial sum that
is at most sum |t_e|; with the product's rounding
    |got - exact| <= (n + 2) 2^-53 sum |t_e|.
`exact` is the rational sum of the exact addends (fractions.Fraction), rounded once to double; the tests hold both the
library and the restatement's own frame-order double sums to this bound, on every element where D <= 5 and on a fixed random
sample of 40 elements per accumulator above.

DEVICE ROUTE AGAINST RESTATEMENT.  The two need not sum the same addends: the device's Gaussian posteriors are within
fmllr_cases.post_bound of the restatement's.  carried_bound carries that bound through the sums - sum over the entries of
post_bound |x|^k - and adds both sides' summation bound; the routes are held to it in double.

IN THE FILE the values are floats (AccumDiagGmm::Write converts), and the device route and the restatement are to agree
elementwise to equal or adjacent floats; the count of unequal elements is printed.  That is a statement relative to the VALUE
|sum t_e|, where the bounds above are relative to sum |t_e|.  With stage A1's posteriors (the device library's expf: 5 % of
them 1 - 3 float ulps from the restatement's) mean_acc elements whose addends cancel, sum |t_e| / |sum t_e| of 76 - 146, were
2 - 4 float ulps apart.  The route therefore takes its posteriors from kh_gmm_acc_component_posteriors, whose exp and log are
the float of the double function, as the restatement states them (ComponentPosteriorsKernel<true> where A1 is <false>; the one
statement of both is the header of csrc/kh_gmmstats.h); what is left between the two routes is the summation order, (n + 2) 2^-53
sum |t_e| each, which moves a float by more than one ulp only under cancellation by 2^28 / n."""
from fractions import Fraction

import numpy as np

CHUNK = 256            # kChunk, csrc/kh_gmmacc.hip: entries of a pdf per chunk
MAX_DIM = 127          # kMaxD
TILE_DIMS = [1, 2, 7, 8, 13, 40]
TILE_SIZES = [1, 2, 15, 16, 17, 33, 2, 16, 1]
TILE_COUNTS = [3, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 0, 1, 4]


def entries(frames, pdf_offsets, weights=None):
    """CSR entry list of `frames` (a list over rows of lists of pdfs): weight 1 unless given per entry."""
    off = np.asarray(pdf_offsets, np.int64)
    feo = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    pdf = np.asarray([p for f in frames for p in f], np.int32)
    goff = np.zeros(len(pdf) + 1, np.int64)
    if len(pdf):
        goff[1:] = np.cumsum(off[pdf + 1] - off[pdf])
    w = np.ones(len(pdf), np.float32) if weights is None else np.asarray(weights, np.float32)
    return dict(feo=feo, pdf=pdf, weight=w, goff=goff)


def tile_case(dim, seed, sizes=TILE_SIZES, counts=TILE_COUNTS):
    """Inputs of kh_gmm_acc_stats made directly (the call takes explicit Gaussian posteriors): pdfs of 1, 2, 15, 16, 17 and 33
    Gaussians with 0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 entries; frames of 0, 1 and 3 entries, the first
    with two entries of one pdf; an entry of weight 0 (all its posteriors 0) and one of weight -0.5.  The frames' rows scale
    per dimension over [0.25, 4].  -> (pdf_offsets, feats [T, dim], ent, gauss_post)"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pool = np.repeat(np.arange(len(sizes)), counts)
    rng.shuffle(pool)
    pool = pool.tolist()
    big = int(np.argmax(counts))
    pool.remove(big)
    pool.remove(big)
    frames = [[big, big, pool.pop()]]
    while pool:
        k = min(len(pool), int(rng.choice([0, 1, 1, 1, 3])))
        frames.append([pool.pop() for _ in range(k)])
    frames += [[], []]
    ent = entries(frames, off)
    E = len(ent["pdf"])
    assert E == sum(counts) and {0, 1, 3} <= set(np.diff(ent["feo"]).tolist())
    w = rng.choice([1.0, 1.0, 1.0, 0.5, 0.25], E).astype(np.float32)
    w[5], w[9] = 0.0, -0.5
    ent["weight"] = w
    feats = (rng.standard_normal((len(frames), dim)) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), dim)) + 0.5).astype(np.float32)
    post = np.zeros(int(ent["goff"][-1]), np.float32)
    for e in range(E):
        n = int(ent["goff"][e + 1] - ent["goff"][e])
        p = rng.dirichlet(np.full(n, 0.7)).astype(np.float32)
        post[int(ent["goff"][e]):int(ent["goff"][e + 1])] = p * w[e]          # posteriors.Scale(weight)
    return off, feats, ent, post


def pdf_entries(ent, num_pdfs):
    """Per pdf, its entries in entry order."""
    out = [[] for _ in range(num_pdfs)]
    for e, p in enumerate(ent["pdf"]):
        out[int(p)].append(e)
    return out


def entry_rows(ent):
    return np.repeat(np.arange(len(ent["feo"]) - 1), np.diff(ent["feo"]))


def exact_element(which, g_local, d, es, rows, feats, ent, post):
    """(exact sum rounded once, sum |t_e| as a Fraction, n) of one element: which = "occ" | "mean_acc" | "var_acc"."""
    s, a = Fraction(0), Fraction(0)
    for e in es:
        t = Fraction(float(post[int(ent["goff"][e]) + g_local]))
        if which != "occ":
            x = Fraction(float(feats[rows[e], d]))
            t *= x if which == "mean_acc" else x * x
        s += t
        a += abs(t)
    return float(s), a, len(es)


def check_bound(acc, pdf_offsets, feats, ent, post, seed, label=""):
    """Hold acc's occ / mean_acc / var_acc (those not None) to the bound: every element where D <= 5, else 40 per accumulator.
    Returns the worst error / bound."""
    off = np.asarray(pdf_offsets, np.int64)
    D = feats.shape[1]
    per_pdf, rows = pdf_entries(ent, len(off) - 1), entry_rows(ent)
    rng = np.random.default_rng(seed)
    pdf_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    worst = 0.0
    for which in ("occ", "mean_acc", "var_acc"):
        if acc[which] is None:
            continue
        dims = [0] if which == "occ" else range(D)
        if D <= 5:
            picks = [(g, d) for g in range(int(off[-1])) for d in dims]
        else:
            picks = [(int(rng.integers(0, off[-1])), int(rng.integers(0, len(dims)))) for _ in range(40)]
        for g, d in picks:
            pdf = int(pdf_of[g])
            exact, mag, n = exact_element(which, g - int(off[pdf]), d, per_pdf[pdf], rows, feats, ent, post)
            got = float(acc[which][g] if which == "occ" else acc[which][g, d])
            bound = Fraction(n + 2) * Fraction(2) ** -53 * mag
            err = abs(Fraction(got) - Fraction(exact))
            assert err <= bound, (label, which, g, d, got, exact, float(bound))
            if n == 0:
                assert got == 0.0
            if bound:
                worst = max(worst, float(err / bound))
    return worst


def carried_bound(pdf_offsets, stats_feats, ent, ref_post, flags=7):
    """Per element, how far sums over posteriors within fmllr_cases.post_bound of ref_post may be from the restatement's:
    sum_e post_bound_e |x_e|^k, plus (n + 2) 2^-53 sum |t_e| for each side's own summation (the device's addends are within
    1 + 2^-20 of the restatement's).  -> dict(occ, mean_acc, var_acc), None where the flags exclude."""
    import fmllr_cases as FC
    off = np.asarray(pdf_offsets, np.int64)
    D = stats_feats.shape[1]
    pb = FC.post_bound(ref_post, ent["goff"])
    ng = int(off[-1])
    out = dict(occ=np.zeros(ng), mean_acc=np.zeros((ng, D)) if flags & 1 else None, var_acc=np.zeros((ng, D)) if flags & 2 else None)
    mag = dict(occ=np.zeros(ng), mean_acc=np.zeros((ng, D)), var_acc=np.zeros((ng, D)))
    rows = entry_rows(ent)
    for e in range(len(ent["pdf"])):
        g0, g1 = int(off[ent["pdf"][e]]), int(off[ent["pdf"][e] + 1])
        q, p = pb[int(ent["goff"][e]):int(ent["goff"][e + 1])], np.abs(ref_post[int(ent["goff"][e]):int(ent["goff"][e + 1])].astype(np.float64))
        x = np.abs(stats_feats[rows[e]].astype(np.float64))
        for k, xs in (("occ", None), ("mean_acc", x), ("var_acc", x * x)):
            if out[k] is not None:
                out[k][g0:g1] += q if xs is None else np.outer(q, xs)
                mag[k][g0:g1] += p if xs is None else np.outer(p, xs)
    n = np.repeat(np.bincount(ent["pdf"], minlength=len(off) - 1), np.diff(off)).astype(np.float64)
    for k in out:
        if out[k] is not None:
            unit = 2.0 * (n + 2.0) * 2.0 ** -53 * (1.0 + 2.0 ** -20)
            out[k] = 1.0001 * (out[k] + (unit if k == "occ" else unit[:, None]) * mag[k])          # 1.0001: this function's own rounding
    return out


def check_carried(got, ref, bound, label=""):
    """The device route's doubles against the restatement's, within carried_bound; prints the worst error / bound."""
    for k in ("occ", "mean_acc", "var_acc"):
        assert (got[k] is None) == (ref[k] is None) == (bound[k] is None), k
        if ref[k] is not None:
            err = np.abs(np.asarray(got[k], np.float64) - ref[k])
            print(label, k, "worst error / carried bound", float((err / np.maximum(bound[k], 1e-300)).max()))
            assert (err <= bound[k]).all(), (label, k)


def adjacent_floats(a, b):
    """a, b float32 arrays: (all equal or adjacent, the number unequal)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ok = (a == b) | (b == np.nextafter(a, np.float32(np.inf))) | (b == np.nextafter(a, np.float32(-np.inf)))
    return bool(ok.all()), int((a != b).sum())


def compare_written(got, want, label=""):
    """Accumulators as read from a file against the restatement's (as_written): floats equal or adjacent; prints the count."""
    for k in ("occ", "mean_acc", "var_acc"):
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            ok, n = adjacent_floats(got[k], want[k])
            print(label, k, "unequal floats:", n, "of", np.asarray(want[k]).size)
            assert ok, (label, k)
    assert got["flags"] == want["flags"] and got["dim"] == want["dim"]
    assert np.array_equal(got["pdf_offsets"], want["pdf_offsets"])


def e2e_utterances(oracle):
    """fmllr_cases.e2e_case as a training job: the model, tid2pdf, and per utterance (key, features, posterior, alignment)."""
    import fmllr_cases as C
    am, feats, utt, spk, posts, tid2pdf = C.e2e_case(oracle)
    ali = C.e2e_alignment(posts)
    utts = [("utt%d" % u, feats[utt[u]:utt[u + 1]], posts[utt[u]:utt[u + 1]], ali[utt[u]:utt[u + 1]]) for u in range(len(utt) - 1)]
    return am, tid2pdf, utts


def second_features(mat, dim, seed):
    """Other features for the same rows (the two-feature route): a fixed random projection to `dim` dimensions."""
    rng = np.random.default_rng(seed)
    return (mat.astype(np.float64) @ rng.standard_normal((mat.shape[1], dim)) / 3.0).astype(np.float32)
