"""Cases, the plan and the derived bound for the LDA statistics tests (csrc/kh_lda.hip, tests/lda_restatement.py).

THE BOUND.  An item is an entry whose weight is not zero; w and x are floats widened to double.
  zero[c]       sums t_i = w_i                over the class's items,
  first[c][d]   sums t_i = w_i x_i[d]         over the class's items; the product of two widened floats is exact (48 bits),
  second[a, b]  sums t_i = (w_i x_i[a]) x_i[b] over ALL items; the inner product is exact, the outer one rounds once (72
                bits), or not at all inside a fused multiply-add.
Whatever the order of the n - 1 additions (the library: per slice in item order by matrix-core fused multiply-adds, the
slices in slice order, the segments in order; per class in chunks; the restatement: item by item) each rounds once,
relative to a partial sum that is at most sum |t_i|; with the products' roundings, together at most 2^-53 sum |t_i|, and
the one of `exact`,
    |got - exact| <= (n + 2) 2^-53 sum |t_i|,
n the number of items that reach the element: all items for `second`, the class's for `first` and `zero`.  This is
tests/mllt_cases.py's derivation with another addend.  Because w and x enter exactly, a staged operand that is one float
ulp off moves an element by about 2^-24 sum |t_i| / sqrt(n), orders of magnitude over the bound.

zero is additionally BIT-EQUAL to the restatement under a condition the cases here meet: every weight is a multiple of
2^-10 and the sum of their magnitudes is below 2^40, so every partial sum in any order is a multiple of 2^-10 below 2^40 -
at most 50 bits - and no addition rounds.

EXACT SUMS.  math.fsum returns the correctly rounded sum of its arguments.  w x[d] is an exact double.  For `second`,
P = w x[a] is exact in double and is split (Veltkamp) into hi + lo of at most 26 bits each, so hi x[b] and lo x[b] are exact
doubles and t = hi x[b] + lo x[b] exactly (mllt_cases.exact_elements, whose o o product is here (w x[a]) and whose weight
is x[b]).  The rational forms use fractions.Fraction; tests/test_lda_restatement.py holds the two equal on a small case,
and the GPU tests use the rational one wherever D <= 5.

THE PLAN.  plan restates the library's rule from the exported constants: a segment of n items is cut into slices of
CHUNK * max(1, ceil(n / (CHUNK * MAX_SLICES))) items; workgroups = slices * S (S + 1) / 2 with S = ceil(D / 64) super tiles;
passes = ceil(slices / min(slices, floor(limit / (8 Q))))."""
import math
from fractions import Fraction

import numpy as np

import mllt_cases as MC

F32, F64 = np.float32, np.float64
CHUNK = 256            # kChunk, csrc/kh_lda.hip
MAX_SLICES = 256       # kMaxSlices
MAX_DIM = 512          # kMaxD
DIMS = [1, 2, 15, 16, 17, 31, 32, 33, 117, MAX_DIM]
ITEM_COUNTS = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
NUM_CLASSES = 5
EMPTY_CLASS = 1        # no entry of kernel_case names it
DEFAULT_LIMIT = 1 << 30


def slice_len(n):
    return CHUNK * max(1, -(-n // (CHUNK * MAX_SLICES)))


def plan(segment_items, dim, limit=DEFAULT_LIMIT):
    """(slices, workgroups, passes) of a call whose segments hold segment_items items."""
    slices = sum(-(-n // slice_len(n)) for n in segment_items if n)
    if slices == 0:
        return 0, 0, 0
    st = -(-dim // 64)
    per_pass = min(slices, limit // (8 * (dim * (dim + 1) // 2)))
    return slices, slices * (st * (st + 1) // 2), -(-slices // per_pass)


def segment_items(ent, segments):
    """Items (nonzero weights) per segment."""
    feo, w = np.asarray(ent["feo"]), np.asarray(ent["weight"])
    return [int((w[int(feo[a]):int(feo[b])] != 0).sum()) for a, b in zip(segments[:-1], segments[1:])]


def kernel_case(dim, n_items, seed, num_classes=NUM_CLASSES):
    """Inputs of kh_lda_acc_stats made directly: frames of 0, 1 and 3 entries (the first frame: two entries on different
    pdfs; three-entry frames name three different pdfs), no entry on EMPTY_CLASS, exactly n_items weights that are not zero -
    multiples of 2^-10 in (0, 2], about a fifth of them negative - and the other weights 0.0 and -0.0 in turn.  The
    features scale per dimension over [0.25, 4].  -> dict(feats, ent, num_classes)"""
    rng = np.random.default_rng(seed)
    usable = [c for c in range(num_classes) if c != EMPTY_CLASS]
    frames = [[usable[0], usable[-1]], usable[:3], [usable[1]]]
    while sum(len(f) for f in frames) < n_items + 12 or len(frames) < 6:
        k = int(rng.choice([0, 1, 1, 1, 3]))
        frames.append(sorted(int(c) for c in rng.choice(usable, k, replace=False)))
    frames += [[], []]
    feo = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    pdf = np.asarray([p for f in frames for p in f], np.int32)
    E = len(pdf)
    assert {0, 1, 3} <= set(np.diff(feo).tolist())
    w = np.zeros(E, F32)
    w[1::2] = F32(-0.0)
    keep = np.sort(rng.choice(E, n_items, replace=False))
    w[keep] = (rng.integers(1, 2049, n_items) * rng.choice([1.0, 1.0, 1.0, 1.0, -1.0], n_items) / 1024.0).astype(F32)
    assert int((w != 0).sum()) == n_items and (n_items == E or (np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all()))
    feats = (rng.standard_normal((len(frames), dim)) * np.exp(rng.uniform(math.log(0.25), math.log(4.0), dim)) + 0.5).astype(F32)
    return dict(feats=feats, ent=dict(feo=feo, pdf=pdf, weight=w), num_classes=num_classes)


def entry_rows(ent):
    return np.repeat(np.arange(len(ent["feo"]) - 1), np.diff(ent["feo"]))


def items_of(feats, ent):
    """The items in entry order -> (x [n, D] float32, w [n] float32, class [n])."""
    w = np.asarray(ent["weight"], F32)
    nz = np.nonzero(w != 0)[0]
    return np.asarray(feats, F32)[entry_rows(ent)[nz]], w[nz], np.asarray(ent["pdf"])[nz]


def restate(feats, ent, num_classes, into=None):
    """The restatement's accumulator of an entry list (no pruning)."""
    import lda_restatement as L
    acc = into if into is not None else L.init(L.empty(), num_classes, feats.shape[1])
    rows = entry_rows(ent)
    for e in range(len(ent["pdf"])):
        if ent["weight"][e] != 0.0:
            L.accumulate(acc, feats[rows[e]], int(ent["pdf"][e]), ent["weight"][e])
    return acc


def restate_zero(ent, num_classes):
    """The counts alone, as the restatement adds them: zero_acc_(class_id) += weight, entry by entry."""
    zero = np.zeros(num_classes, F64)
    for c, w in zip(np.asarray(ent["pdf"]).tolist(), np.asarray(ent["weight"], F32)):
        if w != 0.0:
            zero[c] += F64(w)
    return zero


def big_case(dim, n_items, seed, num_classes=NUM_CLASSES):
    """n_items frames of one entry each, every weight an item (kernel_case without its Python loop, for large counts)."""
    rng = np.random.default_rng(seed)
    usable = np.asarray([c for c in range(num_classes) if c != EMPTY_CLASS], np.int32)
    pdf = usable[rng.integers(0, len(usable), n_items)]
    w = (rng.integers(1, 2049, n_items) * rng.choice([1.0, 1.0, 1.0, 1.0, -1.0], n_items) / 1024.0).astype(F32)
    feats = (rng.standard_normal((n_items, dim)) * np.exp(rng.uniform(math.log(0.25), math.log(4.0), dim)) + 0.5).astype(F32)
    return dict(feats=feats, ent=dict(feo=np.arange(n_items + 1, dtype=np.int64), pdf=pdf, weight=w), num_classes=num_classes)


def zero_is_exact(w):
    """The condition under which every order of adding the weights is exact (the head of this file)."""
    w = np.asarray(w, F64)
    return bool((w * 1024 == np.round(w * 1024)).all()) and float(np.abs(w).sum()) < 2.0 ** 40


# ---- exact sums: lists of (sum, sum |t|), floats (fsum) or Fractions (rational)
def exact_second(x, w, picks, rational=False):
    """picks: [(a, b)], a >= b."""
    if rational:
        out = []
        for a, b in picks:
            s, m = Fraction(0), Fraction(0)
            for i in range(len(w)):
                t = Fraction(float(w[i])) * Fraction(float(x[i, a])) * Fraction(float(x[i, b]))
                s += t
                m += abs(t)
            out.append((s, m))
        return out
    x64, w64 = np.asarray(x, F32).astype(F64), np.asarray(w, F32).astype(F64)
    out = []
    for a, b in picks:
        wx = w64 * x64[:, a]                                                 # exact
        hi, lo = MC._split(wx)
        ahi, alo = MC._split(np.abs(wx))                                     # ahi + alo = |wx| exactly, whatever alo's sign
        xb = x64[:, b]
        out.append((math.fsum(np.concatenate([hi * xb, lo * xb])), math.fsum(np.concatenate([ahi * np.abs(xb), alo * np.abs(xb)]))))
    return out


def exact_first(x, w, cls, picks, rational=False):
    """picks: [(c, d)] -> per pick (sum, sum |t|, n) over the class's items; d = -1: the count zero[c]."""
    x64, w64 = np.asarray(x, F32).astype(F64), np.asarray(w, F32).astype(F64)
    out = []
    for c, d in picks:
        sel = np.nonzero(cls == c)[0]
        t = w64[sel] * (x64[sel, d] if d >= 0 else 1.0)                     # exact doubles
        if rational:
            fr = [Fraction(float(v)) for v in t]
            out.append((sum(fr, Fraction(0)), sum((abs(v) for v in fr), Fraction(0)), len(sel)))
        else:
            out.append((math.fsum(t), math.fsum(np.abs(t)), len(sel)))
    return out


def second_picks(dim, seed, samples=60):
    """Every packed element where dim <= 5; else sampled ones with the last packed element, a diagonal-tile element off the
    diagonal, the last diagonal element's neighbour, and - from dim 17 - an off-diagonal-tile element."""
    r, c = np.tril_indices(dim)
    if dim <= 5:
        return list(zip(r.tolist(), c.tolist()))
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(r), samples)
    picks = set(zip(r[k].tolist(), c[k].tolist())) | {(dim - 1, dim - 1), (dim - 1, 0), (min(dim - 1, 5), 2), (dim - 1, dim - 2)}
    if dim > 16:
        picks |= {(dim - 1, 3), (16, 15)}
    if dim > 70:                                                             # the second super tile: its corner, its diagonal tile
        picks |= {(64, 63), (dim - 1, 64), (70, 65)}
    return sorted(picks)


def first_picks(dim, num_classes, seed, samples=6):
    """Every (class, d) and every count where dim <= 5; else every count and per class sampled columns with the last."""
    if dim <= 5:
        return [(c, d) for c in range(num_classes) for d in range(-1, dim)]
    rng = np.random.default_rng(seed)
    return [(c, int(d)) for c in range(num_classes) for d in [-1] + sorted(set(rng.integers(0, dim, samples).tolist()) | {dim - 1})]


def _hold(got, s, m, n, label):
    bound = Fraction(n + 2) * Fraction(2) ** -53 * Fraction(m)
    err = abs(Fraction(float(got)) - Fraction(s))
    assert err <= bound, (label, float(got), float(s), float(err), float(bound))
    if n == 0:
        assert got == 0.0, label
    return float(err / bound) if bound else 0.0


def check_bound(acc, x, w, cls, seed, label=""):
    """Hold an accumulator to the bound on second_picks and first_picks.  Returns the worst error / bound."""
    dim, nc = int(acc["dim"]), int(acc["num_classes"])
    n = len(w)
    rational = dim <= 5 and n <= 4 * CHUNK
    worst = 0.0
    sp = second_picks(dim, seed)
    for (a, b), (s, m) in zip(sp, exact_second(x, w, sp, rational)):
        worst = max(worst, _hold(acc["second"][a * (a + 1) // 2 + b], s, m, n, (label, "second", a, b)))
    fp = first_picks(dim, nc, seed)
    for (c, d), (s, m, nk) in zip(fp, exact_first(x, w, cls, fp, rational)):
        got = acc["zero"][c] if d < 0 else acc["first"][c, d]
        worst = max(worst, _hold(got, s, m, nk, (label, "first" if d >= 0 else "zero", c, d)))
    return worst
