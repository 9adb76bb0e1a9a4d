"""Generators and derived bounds for the fMLLR estimation tests (csrc/kh_fmllr.hip, tests/fmllr_restatement.py).

THE A1 BOUNDS.  Device and restatement compute, from bit-identical float32 scores f_i of a pdf of n Gaussians,
    x_i = fl32(f_i - max)            identical on both sides
    e_i = EXP(x_i)                   device: expf of the device math library, 1 ulp; restatement: the correctly rounded float
    s   = e_1 + ... + e_n            float additions in Gaussian order on both sides
    p_i = fl32(fl32(e_i * fl32(1.0 / s)) * w),     like = fl32(max + LOG(s))     LOG: 1 ulp / correctly rounded
With u = 2^-24 and ulp32(v) <= 2 u |v|:  the two e_i differ by at most 1.5 ulp = 3 u relative.  Each computed s is the exact
sum of its own (positive) terms within (n - 1) u relative, so the two s differ by at most 3 u + 2 (n - 1) u.  The quotient, the
product with it and the product with w round once each on each side: 6 u.  Together
    |p_dev - p_ref| <= (3 + 3 + 2 (n - 1) + 6) u |p| = (2 n + 10) u |p|,
taken with a factor 1.01 for the second-order terms, plus 2^-126: below the smallest normal float neither side's e_i has a
relative accuracy.  For the score, log s differs by the relative difference of s, (2 n + 1) u, plus 1.5 ulp32(ln n) for the
two logarithms (ln s <= ln n; n = 1 gives s = 1 and log s = 0 on both sides), and the final addition rounds once on each
side: ulp32 of the result, taken at |ref| plus the rest so that a binade edge is covered.

THE B BOUND is the issue's: per element |err| <= (n + 2) 2^-53 sum |addend| with n merged frames, which holds for any
summation order.  The reference sums are formed in x87 extended precision (64-bit significand): an addend b x_r x_c is a
product of three floats (72 bits) and rounds once at 2^-64, the n additions once each, so the reference is within
(n + 1) 2^-64 sum |addend| of the exactly rounded sum - 1/2048 of the bound's unit per frame, inside the "+ 2" for the
n <= 1100 used here.  It serves the large dimensions, where rational arithmetic over every element would take minutes;
test_gpu_fmllr.py holds the device to the issue's bound against exactly rounded sums directly for EVERY element of K and G
at D <= 5 and for a sample of 40 G and 40 K elements at each larger D.

THE END-TO-END TOLERANCE is measured on the CPU, from the restatement alone (never from device output): the committed case
is estimated three times - as stated; with the merged frames added in reverse and every inverse by a Cholesky solve; and with
the Gaussian posteriors multiplied by 1 +- post_rel_bound(n) with random signs (seed TOL_SEED).  MEASURED_DIFF[type] is the
larger element-wise difference of the float transforms from the unperturbed run; the tests allow 4 x that (the device
differs in both ways at once, and the perturbation is a sample, not a maximum), and never less than 1 ulp32 of the row's
largest element.  test_fmllr_restatement.py measures again and holds the figures below to within a factor 2."""
import math

import numpy as np

import fmllr_restatement as R
import gmm_cases

FRAME_CHUNK = 256      # kFrameChunk, csrc/kh_fmllr.hip: merged frames per workgroup of FmllrAccumulateKernel
MAX_DIM = 63           # kMaxD, csrc/kh_fmllr.hip
U = 2.0 ** -24


def post_rel_bound(n):
    return 1.01 * (2 * np.asarray(n, np.float64) + 10) * U


def post_bound(ref_post, goff):
    """Elementwise bound for A1's posteriors: entry sizes from goff."""
    n = np.repeat(np.diff(goff), np.diff(goff))
    return post_rel_bound(n) * np.abs(ref_post.astype(np.float64)) + 2.0 ** -126


def like_bound(ref_like, goff):
    n = np.diff(goff).astype(np.float64)
    rest = (2 * n + 1) * U + 1.5 * np.spacing(np.log(n).astype(np.float32)).astype(np.float64)
    return rest + np.spacing((np.abs(ref_like.astype(np.float64)) + rest).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------- models and features
def model(sizes, dim, seed, oracle):
    """dict(gconsts, means_invvars, inv_vars, pdf_offsets, means, vars) of a gmm_cases.clustered_model."""
    rng = np.random.default_rng(seed)
    am = gmm_cases.clustered_model(sizes, dim, rng)
    g, mi, iv = gmm_cases.model_params(am, oracle)
    return dict(gconsts=g, means_invvars=mi, inv_vars=iv, pdf_offsets=am["pdf_offsets"], means=am["means"], vars=am["vars"],
                weights=am["weights"])


def other_model(am, seed):
    """Another model with the same Gaussian counts (the two-model case of gmm-est-fmllr-gpost)."""
    rng = np.random.default_rng(seed)
    return dict(am, means_invvars=(am["means_invvars"] + 0.1 * rng.standard_normal(am["means_invvars"].shape)).astype(np.float32),
                inv_vars=(am["inv_vars"] * np.exp(0.1 * rng.standard_normal(am["inv_vars"].shape))).astype(np.float32))


def scaled_frames(rng, T, dim):
    """N(0, 1) frames times a per-dimension scale in [0.25, 4]."""
    return (rng.standard_normal((T, dim)) * np.exp(rng.uniform(math.log(0.25), math.log(4.0), dim))).astype(np.float32)


A1_SIZES = [1, 2, 63, 64, 65, 129]


def a1_case(oracle, dim=13, seed=11):
    """Pdf sizes 1, 2, 63, 64, 65, 129; frames with 1 and 3 entries, one with none, weights 0 and negative."""
    am = model(A1_SIZES, dim, seed, oracle)
    rng = np.random.default_rng(seed + 1)
    feats = gmm_cases.frames(rng, 12, dim)
    feats[7:] = scaled_frames(rng, 5, dim)[:]
    posts = [[(0, 1.0)], [(1, 0.5), (2, 0.25), (5, 0.25)], [], [(3, 1.0)], [(4, 0.0)], [(0, 0.3), (4, 0.5), (5, 0.2)],
             [(5, 1.0)], [(2, 1.0)], [(3, 0.7), (4, 0.2), (5, 0.1)], [(1, -0.5)], [(4, 1.0)], [(2, 0.125), (3, 0.5), (5, 0.375)]]
    return am, feats, posts


def a2_case(oracle, dim=13, seed=21):
    """Given Gaussian posteriors on 3 speakers / 7 utterances (speaker 1: four unequal utterances of 1, 3, 4 and 2 rows, the
      merged frame of rows 16-19 across the boundary of its last two) with every merging case:
      rows 1-2 identical (two), rows 4-6 identical (three), rows 8|9 identical across the boundary of speaker 0's two
      utterances, speaker 1 starts with an all-zero row, row 14's only entry sums to zero (count 0), rows 16 and 18 identical
      with row 17 between them carrying no entries (merged: the reference never sees row 17), rows 20|21 identical across a
      SPEAKER boundary (not merged)."""
    am = model([3, 1, 4, 2], dim, seed, oracle)
    rng = np.random.default_rng(seed + 1)
    T = 24
    feats = gmm_cases.frames(rng, T, dim)
    feats[2] = feats[1]
    feats[5] = feats[4]
    feats[6] = feats[4]
    feats[9] = feats[8]
    feats[11] = 0.0
    feats[18] = feats[16]
    feats[19] = feats[16]      # ... and row 19, across the boundary between the third and fourth of speaker 1's utterances
    feats[21] = feats[20]
    utt = np.array([0, 9, 11, 12, 15, 19, 21, 24], np.int32)
    spk = np.array([0, 2, 6, 7], np.int32)
    sizes = np.diff(am["pdf_offsets"])
    gposts = []
    for t in range(T):
        if t in (3, 17):
            gposts.append([])
            continue
        pdfs = sorted(rng.choice(4, size=int(rng.integers(1, 4)), replace=False).tolist())
        gposts.append([(p, rng.uniform(0.0, 1.0, sizes[p]).astype(np.float32)) for p in pdfs])
    gposts[14] = [(3, np.array([0.5, -0.5], np.float32))]
    return am, feats, utt, spk, gposts


def gpost_entries(gposts):
    feo = np.zeros(len(gposts) + 1, np.int64)
    pdf, vec = [], []
    for t, fr in enumerate(gposts):
        for p, v in fr:
            pdf.append(p)
            vec.append(np.asarray(v, np.float32))
        feo[t + 1] = len(pdf)
    goff = np.zeros(len(pdf) + 1, np.int64)
    goff[1:] = np.cumsum([len(v) for v in vec])
    ent = dict(feo=feo, pdf=np.asarray(pdf, np.int32), weight=np.ones(len(pdf), np.float32), goff=goff)
    return ent, (np.concatenate(vec) if vec else np.zeros(0, np.float32))


B_DIMS = [1, 4, 5, 15, 16, 17, 39, 40, 63]
B_FRAMES = [1, 3, 4, 5, FRAME_CHUNK - 1, FRAME_CHUNK, FRAME_CHUNK + 1, 2 * FRAME_CHUNK + 1]


def b_case(dim, seed, frames=None):
    """Inputs of stage B made directly (the stage takes explicit inputs): one speaker per entry of `frames` merged frames,
    then a speaker without any, then one more of 31 (stage B sees merged frames, not utterances: the speaker of four
    unequal utterances is in a2_case and e2e_case, which pass through kh_fmllr_frame_stats).  Some counts are 0: those frames must add nothing, whatever their a and b.  Rows are picked out of order."""
    rng = np.random.default_rng(seed)
    frames = list(B_FRAMES if frames is None else frames) + [0, 31]
    n = int(sum(frames))
    T = n + 5
    feats = scaled_frames(rng, T, dim)
    run_row = rng.permutation(T)[:n].astype(np.int32)
    a = (rng.standard_normal((n, dim)) * 3).astype(np.float32)
    b = np.exp(rng.standard_normal((n, dim))).astype(np.float32)
    count = rng.uniform(0.5, 1.5, n)
    count[rng.random(n) < 0.1] = 0.0
    spk = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
    return feats, dict(run_row=run_row, spk_run_offsets=spk, a=a, b=b, count=count)


def b_reference(feats, fs):
    """(beta, K, G, K_abs, G_abs, n): sums in extended precision and the sums of |addend| (float64), n = merged frames."""
    assert np.finfo(np.longdouble).nmant >= 63, "x87 extended precision is needed for the reference sums"
    D = feats.shape[1]
    pr, pc = R.packed_index(D)
    S = len(fs["spk_run_offsets"]) - 1
    P = len(pr)
    beta, K, G = np.zeros(S), np.zeros((S, D, D + 1)), np.zeros((S, D, P))
    Ka, Ga, n = np.zeros((S, D, D + 1)), np.zeros((S, D, P)), np.zeros(S, np.int64)
    LD = np.longdouble
    for s in range(S):
        r0, r1 = int(fs["spk_run_offsets"][s]), int(fs["spk_run_offsets"][s + 1])
        live = np.nonzero(fs["count"][r0:r1] != 0.0)[0] + r0
        n[s] = r1 - r0
        if len(live) == 0:
            continue
        xp = np.concatenate([feats[fs["run_row"][live]].astype(np.float64), np.ones((len(live), 1))], axis=1)
        sc = xp[:, pr] * xp[:, pc]                                  # exact: a product of two floats
        a64, b64 = fs["a"][live].astype(np.float64), fs["b"][live].astype(np.float64)
        beta[s] = math.fsum(fs["count"][live])
        K[s] = (a64.T.astype(LD) @ xp.astype(LD)).astype(np.float64)
        G[s] = (b64.T.astype(LD) @ sc.astype(LD)).astype(np.float64)
        Ka[s] = np.abs(a64).T @ np.abs(xp)
        Ga[s] = np.abs(b64).T @ np.abs(sc)
    return beta, K, G, Ka, Ga, n


# ---------------------------------------------------------------- the end-to-end case
E2E_DIM, E2E_SIZES, E2E_MIN_COUNT = 13, [3, 5, 8, 2, 6, 4], 100.0
E2E_UTT_FRAMES = [470, 200, 150, 90, 40, 280, 190, 40]    # speakers: [470] [200 150 90 40: four unequal] [280 190] [40: under the min-count]
E2E_SPK = [0, 1, 5, 7, 8]
E2E_SPK_NAMES = ["spkA", "spkB", "spkC", "spkD"]
TOL_SEED = 77
# max |difference| of the float transforms from the unperturbed run, per update type (measured on the CPU as stated above)
MEASURED_DIFF = {"full": 2.905726432800293e-07, "diag": 1.1920928955078125e-07, "offset": 8.940696716308594e-08, "none": 0.0}
MEASURED_DIFF_PER_UTT = {"full": 7.152557373046875e-07}      # the same with every utterance its own speaker
TYPES = ["full", "diag", "offset", "none"]


def e2e_case(oracle, seed=31):
    """D = 13, 6 pdfs, 4 speakers (the last with 40 frames: under the min-count of 100).  Frames are drawn from the model's
    own Gaussians and distorted per speaker (a diagonal scale in [0.8, 1.25] and an offset), so that there is a transform to
    estimate.  Transition-ids 1 .. 12, pdf = (tid - 1) // 2; most frames carry one id, some two ids of one pdf or of two,
    some none; a few rows repeat the row before."""
    am = model(E2E_SIZES, E2E_DIM, seed, oracle)
    rng = np.random.default_rng(seed + 1)
    off = am["pdf_offsets"]
    utt = np.concatenate([[0], np.cumsum(E2E_UTT_FRAMES)]).astype(np.int32)
    spk = np.asarray(E2E_SPK, np.int32)
    T = int(utt[-1])
    tid2pdf = np.array([-1] + [(t - 1) // 2 for t in range(1, 13)], np.int32)
    feats = np.zeros((T, E2E_DIM), np.float32)
    posts = []
    for s in range(len(spk) - 1):
        scale = np.exp(rng.uniform(math.log(0.8), math.log(1.25), E2E_DIM))
        shift = rng.uniform(-0.5, 0.5, E2E_DIM)
        for t in range(int(utt[spk[s]]), int(utt[spk[s + 1]])):
            p = int(rng.integers(0, 6))
            g = int(rng.integers(off[p], off[p + 1]))
            x = am["means"][g] + np.sqrt(am["vars"][g]) * rng.standard_normal(E2E_DIM)
            feats[t] = (x * scale + shift).astype(np.float32)
            k = rng.random()
            if k < 0.05:
                posts.append([])
            elif k < 0.15:
                q = int(rng.integers(0, 6))
                posts.append([(2 * p + 1, 0.625), (2 * q + 2, 0.375)])
            elif k < 0.2:
                posts.append([(2 * p + 2, 0.5), (2 * p + 1, 0.5)])
            else:
                posts.append([(2 * p + 1 + int(rng.integers(0, 2)), 1.0)])
            if t > int(utt[spk[s]]) and rng.random() < 0.02:
                feats[t] = feats[t - 1]
    return am, feats, utt, spk, posts, tid2pdf


def e2e_alignment(posts):
    """An alignment for the tools' pipeline: the first transition-id of every frame of the case's posteriors (1 where none)."""
    return [int(fr[0][0]) if fr else 1 for fr in posts]


def e2e_model_files(kio, am, path):
    """final.mdl for the end-to-end case: six phones of one emitting state with a self-loop and an exit (transition-ids
    2 p + 1 and 2 p + 2 -> pdf p, phone p + 1), then the AmDiagGmm."""
    n = len(am["pdf_offsets"]) - 1
    topo = dict(phones=list(range(1, n + 1)), phone2idx=[-1] + [0] * n, entries=[[(0, [(0, 0.5), (1, 0.5)]), (-1, [])]])
    triples = [(p + 1, 0, p) for p in range(n)]
    log_probs = np.concatenate([[0.0], np.log(np.tile([0.75, 0.25], n))]).astype(np.float32)
    with open(path, "wb") as f:
        f.write(b"\0B")
        kio.write_transition_model(f, topo, triples, log_probs, True)
        kio.write_am_diag_gmm(f, dict(am, dim=am["means_invvars"].shape[1]), True)


def pdf_posts_of(posts, tid2pdf):
    """api.convert_posterior_to_pdfs restated (ConvertPosteriorToPdfs hmm/posterior.cc:308-332, ascending pdf order)."""
    out = []
    for fr in posts:
        acc = {}
        for tid, w in fr:
            pdf = int(tid2pdf[tid])
            acc[pdf] = np.float32(acc[pdf] + np.float32(w)) if pdf in acc else np.float32(w)
        out.append([(k, float(v)) for k, v in sorted(acc.items()) if v != 0.0])
    return out


def e2e_reference(oracle, per_utt=False, posts=None, types=None):
    """The restatement on the end-to-end case, per update type (per_utt: every utterance its own speaker, "full" only), and the
    two perturbed runs of the tolerance study.  -> dict(case, ent, post, like, fs, stats, ref[type], diff[type])"""
    am, feats, utt, spk, case_posts, tid2pdf = e2e_case(oracle)
    posts = case_posts if posts is None else posts          # (other posteriors on the same frames: the tools' pipeline)
    if per_utt:
        spk = np.arange(len(utt), dtype=np.int32)
    ent = R.entries_of(pdf_posts_of(posts, tid2pdf), am["pdf_offsets"])
    post, like = R.component_posteriors(am, feats, ent)
    fs = R.frame_stats(am, feats, utt, spk, ent, post)
    stats = R.accumulate(feats, fs)
    rng = np.random.default_rng(TOL_SEED)
    n = np.repeat(np.diff(ent["goff"]), np.diff(ent["goff"]))
    post_p = (post * (1.0 + rng.choice([-1.0, 1.0], len(post)) * post_rel_bound(n))).astype(np.float32)
    stats_rev = R.accumulate(feats, fs, reverse=True)
    stats_per = R.accumulate(feats, R.frame_stats(am, feats, utt, spk, ent, post_p))
    ref, diff = {}, {}
    for ty in (types or (["full"] if per_utt else TYPES)):
        kw = dict(update_type=ty, min_count=E2E_MIN_COUNT, num_iters=40)
        ref[ty] = R.update(stats, **kw)
        w_rev = R.update(stats_rev, inverse="chol", **kw)[0]
        w_per = R.update(stats_per, **kw)[0]
        diff[ty] = float(max(np.abs(w_rev.astype(np.float64) - ref[ty][0]).max(), np.abs(w_per.astype(np.float64) - ref[ty][0]).max()))
    return dict(case=(am, feats, utt, spk, posts, tid2pdf), ent=ent, post=post, like=like, fs=fs, stats=stats, ref=ref, diff=diff)


def transform_tolerance(w_ref, update_type, per_utt=False, measured=None):
    """Elementwise tolerance [S, D, D + 1]: 4 x the measured figure, at least 1 ulp32 of the row's largest element.
    measured: the figure of an e2e_reference run on other posteriors (its diff[type]); None: the recorded ones."""
    row_ulp = np.spacing(np.abs(w_ref).max(axis=2).astype(np.float32)).astype(np.float64)[:, :, None]
    if measured is None:
        measured = MEASURED_DIFF_PER_UTT[update_type] if per_utt else MEASURED_DIFF[update_type]
    return np.maximum(4.0 * measured, row_ulp) * np.ones_like(w_ref, dtype=np.float64)


def aux_drop_allowed(W, tol, beta, K, Gp):
    """How far FmllrAuxFuncDiagGmm may fall when the transform W moves by at most tol per element.  With
    f(W) = beta log |det A| + tr(W K^T) - 1/2 sum_d w_d G_d w_d^T (A = W's square part),  the gradient is
    P = beta [A^-T, 0] + K - S, S_d = G_d w_d (FmllrAuxfGradient, fmllr-diag-gmm.cc:510-540), and to first order
    f(W + E) - f(W) = sum P_ij E_ij >= - sum |P_ij| tol_ij.  The second-order terms are bounded by
    1/2 sum_d t_d |G_d| t_d^T (the quadratic) + beta (||A^-1||_F ||t||_F)^2 (log det: |log det(I + X) - tr X| <= ||X||_F^2
    for ||X||_F <= 1/2), t = tol.  f itself is evaluated in double: 1e-12 |f| covers it."""
    D = W.shape[0]
    Gf = R.full_g(Gp, D)
    W64 = W.astype(np.float64)
    Ainv = np.linalg.inv(W64[:, :D])
    P = K - np.stack([Gf[d] @ W64[d] for d in range(D)])
    P[:, :D] += beta * Ainv.T
    first = float((np.abs(P) * tol).sum())
    quad = 0.5 * sum(float(tol[d] @ (np.abs(Gf[d]) @ tol[d])) for d in range(D))
    x = np.linalg.norm(Ainv) * np.linalg.norm(tol[:, :D])
    assert x <= 0.5
    return first + quad + beta * x * x + 1e-12 * abs(R.aux(W64, beta, K, Gf))
