"""Cases and the derived bound for the MLLT statistics tests (csrc/kh_mllt.hip, tests/mllt_restatement.py).

THE BOUND.  An element G_j[a, b] is the sum over the n items (the (entry, Gaussian) pairs whose pruned posterior is not zero)
of addends t_i = w_i[j] o_i[a] o_i[b], with o = fl32(fl32(means_invvars / inv_vars) - x) and w = fl32(inv_vars * p) made in
numpy float32 (IEEE division and subtraction) and widened to double.  o[a] o[b] is exact in double (48 bits); its product
with w rounds once (72 bits), or not at all inside a fused multiply-add.  Whatever the order of the n - 1 additions (the
library: per slice in item order by matrix-core fused multiply-adds, the slices in slice order; the restatement: item by item)
each rounds once, relative to a partial sum that is at most sum |t_i|; with the products' roundings, together at most
2^-53 sum |t_i|, and the one of `exact`,
    |got - exact| <= (n + 2) 2^-53 sum |t_i|.
This is DESIGN.md's derivation for kh_gmm_acc_stats with another addend.  Because o and w enter exactly, a device o or w
that is one float ulp off moves an element by about 2^-24 sum |t_i| / sqrt(n), orders of magnitude over the bound: the bound
is the check on the staging arithmetic (the division above all).

EXACT SUMS.  exact_elements gives `exact` (the rational sum rounded once to double) and sum |t_i| through math.fsum, which
returns the correctly rounded sum of its arguments: P = o[a] o[b] is exact in double and is split (Veltkamp) into hi + lo of
at most 26 bits each, so w hi and w lo are exact doubles and t = w hi + w lo exactly.  exact_elements_rational does the same in
fractions.Fraction; tests/test_mllt_restatement.py holds the two equal on a small case, and the GPU tests use the rational
one wherever D <= 5.

THE PLAN.  slice_plan restates the library's rule from the exported constants: slices of
CHUNK * max(1, ceil(n / (CHUNK * MAX_SLICES))) items; workgroups = slices * ceil(ceil(Q / 16) / 16)."""
import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
CHUNK = 256            # kChunk, csrc/kh_mllt.hip
MAX_SLICES = 256       # kMaxSlices
MAX_DIM = 64           # kMaxD
DIMS = [1, 2, 5, 15, 16, 17, 31, 32, 40, MAX_DIM]
ITEM_COUNTS = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
SIZES = [1, 2, 16, 17]


def slice_plan(n, dim):
    """(slice length, slices, workgroups) of a call with n items."""
    if n == 0:
        return 0, 0, 0
    slice_len = CHUNK * max(1, -(-n // (CHUNK * MAX_SLICES)))
    slices = -(-n // slice_len)
    q = dim * (dim + 1) // 2
    return slice_len, slices, slices * -(-(-(-q // 16)) // 16)


def kernel_case(dim, n_items, seed, sizes=SIZES):
    """Inputs of kh_mllt_acc_stats made directly (the call takes explicit, already pruned posteriors): pdfs of 1, 2, 16 and
    17 Gaussians; frames of 0, 1 and 3 entries, the first with two entries of one pdf; exactly n_items nonzero posteriors,
    about a fifth of them negative, the other slots 0 (whole entries of zeros among them).  The inverse variances scale over
    [0.25, 4], the frames' rows per dimension over [0.25, 4].
    -> dict(off, mi, iv, feats, ent, post)"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    ng = int(off[-1])
    iv = np.exp(rng.uniform(math.log(0.25), math.log(4.0), (ng, dim))).astype(F32)
    mi = (rng.standard_normal((ng, dim)) * 2.0 * iv).astype(F32)
    frames, slots = [[len(sizes) - 1, len(sizes) - 1, 0]], 2 * sizes[-1] + sizes[0]
    while slots < n_items + 24 or len(frames) < 6:
        k = int(rng.choice([0, 1, 1, 1, 3]))
        fr = [int(rng.integers(0, len(sizes))) for _ in range(k)]
        frames.append(fr)
        slots += sum(sizes[p] for p in fr)
    frames += [[], []]
    feo = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    pdf = np.asarray([p for f in frames for p in f], np.int32)
    goff = np.concatenate([[0], np.cumsum(off[pdf + 1] - off[pdf])]).astype(np.int64)
    ent = dict(feo=feo, pdf=pdf, weight=np.ones(len(pdf), F32), goff=goff)
    assert {0, 1, 3} <= set(np.diff(feo).tolist()) and int(goff[-1]) == slots
    post = np.zeros(slots, F32)
    free = np.arange(slots)
    free = free[(free < goff[1]) | (free >= goff[2])]                        # entry 1 stays all zeros
    keep = np.sort(rng.choice(free, n_items, replace=False))
    v = (rng.uniform(0.01, 1.0, n_items) * rng.choice([1.0, 1.0, 1.0, 1.0, -1.0], n_items)).astype(F32)
    post[keep] = v
    assert int((post != 0).sum()) == n_items
    feats = (rng.standard_normal((len(frames), dim)) * np.exp(rng.uniform(math.log(0.25), math.log(4.0), dim)) + 0.5).astype(F32)
    return dict(off=off, mi=mi, iv=iv, feats=feats, ent=ent, post=post)


def entry_rows(ent):
    return np.repeat(np.arange(len(ent["feo"]) - 1), np.diff(ent["feo"]))


def items_of(off, mi, iv, feats, ent, post):
    """The items of a call in entry order then Gaussian order -> (o [n, D], w [n, D]) float32, made as the reference makes
    them (mllt.cc:146-154), and the posteriors [n]."""
    off = np.asarray(off, np.int64)
    slot_entry = np.repeat(np.arange(len(ent["pdf"])), np.diff(ent["goff"]))
    nz = np.nonzero(post != 0)[0]
    e = slot_entry[nz]
    g = off[ent["pdf"][e]] + (nz - ent["goff"][e])
    rows = entry_rows(ent)[e]
    mi, iv = np.asarray(mi, F32), np.asarray(iv, F32)
    mean = (mi[g] / iv[g]).astype(F32)
    o = (mean - np.asarray(feats, F32)[rows]).astype(F32)
    w = (iv[g] * post[nz][:, None]).astype(F32)
    return o, w, post[nz]


def _split(p):
    c = p * 134217729.0                                                      # 2^27 + 1
    hi = c - (c - p)
    return hi, p - hi


def exact_elements(o, w, picks):
    """For (j, a, b) in picks: (the exact sum of w[:, j] o[:, a] o[:, b] rounded once, sum |t| rounded once)."""
    o64, w64 = o.astype(F64), w.astype(F64)
    out = []
    for j, a, b in picks:
        p = o64[:, a] * o64[:, b]
        hi, lo = _split(p)
        ahi, alo = _split(np.abs(p))
        aw = np.abs(w64[:, j])
        out.append((math.fsum(np.concatenate([w64[:, j] * hi, w64[:, j] * lo])), math.fsum(np.concatenate([aw * ahi, aw * alo]))))
    return out


def exact_elements_rational(o, w, picks):
    """The same in rational arithmetic -> (Fraction sum, Fraction sum |t|)."""
    out = []
    for j, a, b in picks:
        s, m = Fraction(0), Fraction(0)
        for i in range(len(o)):
            t = Fraction(float(w[i, j])) * Fraction(float(o[i, a])) * Fraction(float(o[i, b]))
            s += t
            m += abs(t)
        out.append((s, m))
    return out


def picks_of(dim, seed, per_row=30):
    """Every element where dim <= 5, else per_row sampled packed elements of each G_j (the last one always)."""
    a, b = np.tril_indices(dim)
    q = len(a)
    if dim <= 5:
        return [(j, int(a[k]), int(b[k])) for j in range(dim) for k in range(q)]
    rng = np.random.default_rng(seed)
    return [(j, int(a[k]), int(b[k])) for j in range(dim) for k in list(rng.integers(0, q, per_row - 1)) + [q - 1]]


def check_bound(G, o, w, dim, seed, label="", extra=None):
    """Hold G [D, Q] to the bound on picks_of(dim, seed); extra: per pick an allowance added to the bound (a carried bound).
    Returns the worst error / bound."""
    picks = picks_of(dim, seed)
    n = len(o)
    rational = dim <= 5 and n <= 4 * CHUNK
    ex = exact_elements_rational(o, w, picks) if rational else exact_elements(o, w, picks)
    worst = 0.0
    for k, ((j, a, b), (s, m)) in enumerate(zip(picks, ex)):
        got = float(G[j, a * (a + 1) // 2 + b])
        bound = Fraction(n + 2) * Fraction(2) ** -53 * Fraction(m) + (Fraction(float(extra[k])) if extra is not None else 0)
        err = abs(Fraction(got) - Fraction(s))
        assert err <= bound, (label, j, a, b, got, float(s), float(err), float(bound))
        if n == 0:
            assert got == 0.0
        if bound:
            worst = max(worst, float(err / bound))
    return worst


def carried_allowance(o, w, p, p_bound, dim, seed):
    """Per pick of picks_of(dim, seed): how far a sum over posteriors within p_bound [n] of p may move - w = fl32(iv p), so
    |w' - w| <= |w| (p_bound / |p|) (1 + 2^-22) + 2^-22 |w| where p_bound > 0 - times |o[a] o[b]|, plus the other side's own
    summation bound (n + 2) 2^-53 sum |t| (1 + 2^-20)."""
    picks = picks_of(dim, seed)
    o64, w64 = np.abs(o.astype(F64)), np.abs(w.astype(F64))
    rel = np.where(p_bound > 0, p_bound / np.maximum(np.abs(p.astype(F64)), 1e-300) * (1 + 2.0 ** -22) + 2.0 ** -22, 0.0)
    out = []
    for j, a, b in picks:
        t = w64[:, j] * o64[:, a] * o64[:, b]
        out.append(1.0001 * float((rel * t).sum() + (len(o) + 2) * 2.0 ** -53 * (1 + 2.0 ** -20) * t.sum()))
    return out


def margins_hold(log, ulps=4):
    """The condition of the tool tests, on the restatement's own log (rand_prune's log): no draw within `ulps` float ulps of
    the quotient it is compared with, and no |posterior| within `ulps` float ulps of a threshold it is compared with unless
    equal to it.  Under it a device posterior within `ulps` ulps of the restatement's takes the same branch everywhere."""
    for p, thresh, u, q in log:
        if thresh != 0 and p != thresh and abs(p - thresh) <= ulps * float(np.spacing(F32(thresh))):     # threshold 0: no branch
            return False
        if u is not None and abs(u - q) <= ulps * float(np.spacing(F32(q))):
            return False
    return True
