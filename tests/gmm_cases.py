"""Helpers of test_gmm_reference.py (CPU) and test_gpu_gmm_dispatch.py (GPU): the GMM scoring of kh_gmm.hip.

1. Models whose every Gaussian carries weight in its pdf's sum (clustered_model), the pdf-size lists that put the
   fused kernel's tiles and chunk loops on their edges, and models whose per-Gaussian scores a test dictates bit for
   bit (the zero-frame identity).
2. The launch decisions of kh_gmm.hip restated as pure functions of (T, D, M, pdf_offsets, num_cus, env); each cites
   the source line it mirrors.  A test asserts them BEFORE the call, so that a case which drifts out of its branch
   fails loudly instead of passing on another path.
3. The float64 reference of the per-pdf LogSumExp and the error bound of the kernels' arithmetic against it, derived
   below from the operations, never from what the kernels give.

THE BOUND.  Per (frame, pdf) the kernels compute, from the float32 per-Gaussian scores f_i with mx = max f_i and the
kept set {f_i >= cutoff} (all float32, as kaldi-vector.cc:745-763):

    x_i = fl32(f_i - mx)                     -15.95 <= x_i <= 0  (cutoff = mx + log(FLT_EPSILON) = mx - 15.94)
    y_i = fl32(x_i * fl32(log2 e))
    e_i = EXP2(y_i)                          hardware exp2 (V_EXP_F32)
    s   = sum of e_i in float64, Gaussian order
    L   = LOG2(fl32(s))                      hardware log2 (V_LOG_F32)
    r   = fl32(L * fl32(ln 2))
    out = fl32(float64(mx) + float64(r))

and the reference is mx + log(sum exp(f_i - mx)) over the same kept set in float64.  The "CDNA3 Instruction Set
Architecture" reference guide states the accuracy of both V_EXP_F32 and V_LOG_F32 as 1 ULP; that figure is used,
assuming that gfx950 matches it.
With u = 2^-24, the relative error of one term e_i against exp(f_i - mx) is at most

    a. 2^-21                the float subtraction: 1/2 ulp of |x| < 16 (an absolute error of x = a relative one of e)
    b. 15.95 u = 9.5e-7     rounding of the product y: |y| u relative in y, times ln 2 -> |x| u
    c. 15.95 * |fl32(log2 e) / log2 e - 1| = 15.95 * 1.34e-8 = 2.1e-7      the constant as a float
    d. 2^-23                1 ulp of the hardware exp2 (relative: e in (0, 1])

and the relative error of s is at most the largest of its terms' plus n 2^-53 for the float64 additions; a relative
error of s is an absolute error of log s.  Then

    e. 2^-24                s rounded to float (relative)
    f. ulp32(log2 n) ln 2   1 ulp of the hardware log2, L <= log2 n for a pdf of n Gaussians
    g. ulp32(ln n)          r: ln 2 as a float (relative error < u, |r| u <= 1/2 ulp32(r)) and the product's rounding
                            (1/2 ulp32(r)), r <= ln n
    h. 1/2 ulp32(out)       the final rounding (the float64 addition before it: 2^-53 relative, nothing)

c(n) = a + b + c + d + n 2^-53 + e + f + g: 1.82e-6 + ulp32(log2 n) ln 2 + ulp32(ln n), that is 2.63e-6 for n = 128
(f = 3.3e-7, g = 4.8e-7), 1.82e-6 for n = 1 and 3.43e-6 for n = 12289.  The tests hold the kernels to TWICE the derived
value, and take the ulp of h at |ref| + 2 c(n) so that a result pushed over a binade edge is still covered:

    |out - ref| <= 1/2 ulp32(|ref| + 2 c(n)) + 2 c(n).

The CPU oracle (float subtraction, libm expf, double log) has terms a, d (expf is within 1 ulp) and h only: it must
stay inside the same bound, which test_gmm_reference.py checks before any GPU test relies on the reference."""
import math

import numpy as np

KGT = 128                  # kGT, kh_gmm.hip:208: Gaussians per tile of the fused kernel
KTILE_M = 64               # kTileM, kh_gmm.hip:45
LSE_LDS_FLOATS = 12288     # kLseLdsFloats, kh_gmm.hip:138
GEMM_THRESHOLD = 1 << 22   # kh_gmm.hip:494 and :550

# ---------------------------------------------------------------- pdf-size lists
# One unit = 16 pdfs, 678 Gaussians.  Alone it tiles as [1 7 8 9 16 17] [100] [128] [1 127] [127 1] [64 64] [3 5]:
# a pdf of 1 directly after one of 128, a tile that is one pdf of 128, tiles of exactly 128 made of 1 + 127, 127 + 1
# and 64 + 64, a pdf ending on the chunk length (8), one past it (9), two chunks (16), two and one (17), 13 chunks
# (100) and all 16 chunks (128).  Repeated, the unit's last two pdfs join the next unit's first six.
EDGE_UNIT = [1, 7, 8, 9, 16, 17, 100, 128, 1, 127, 127, 1, 64, 64, 3, 5]
EDGE_SIZES = EDGE_UNIT * 6                                          # 4068 Gaussians, 37 tiles: >= 4 per share of 8
EDGE_SIZES_129 = EDGE_SIZES[:40] + [129] + EDGE_SIZES[40:]          # one pdf too large for a tile
EDGE_SIZES_SMALL = list(EDGE_UNIT)                                  # 7 tiles: fewer than the largest split


def offsets_of(sizes):
    off = np.zeros(len(sizes) + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    return off


def uneven_sizes(num_mix, rng, first=(200, 1, 129, 5)):
    """Pdf sizes summing to num_mix: `first`, then sizes drawn from 1..40."""
    sizes = list(first)
    left = num_mix - sum(sizes)
    assert left >= 0
    while left > 0:
        n = min(int(rng.integers(1, 41)), left)
        sizes.append(n)
        left -= n
    return sizes


# ---------------------------------------------------------------- models
def clustered_model(sizes, dim, rng, spread=None):
    """Each pdf a cluster: centre ~ N(0, I), its Gaussians' means = centre + spread N(0, I), variances
    exp(spread N), weights Dirichlet(2), so that every Gaussian of a pdf carries weight in the pdf's sum on a good
    share of N(0, I) frames.  spread = 0.2 up to 13 dimensions and 0.2 sqrt(13 / dim) above: the scores of a pdf's
    Gaussians on a frame spread like spread * sqrt(dim), and a Gaussian more than ln(bound) = 12 below its pdf's
    maximum is invisible.  (With 0.3 at every dimension the sensitivity condition of test_gmm_reference.py fails:
    measured on 140 frames, the worst Gaussian of the edge models counted on 29 % of them at 13 dimensions, 11 % at
    16 and 1 % at 40; with this spread on 66 % at the least.)"""
    if spread is None:
        spread = 0.2 * min(1.0, math.sqrt(13.0 / dim))
    off = offsets_of(sizes)
    M, P = int(off[-1]), len(sizes)
    centres = rng.standard_normal((P, dim))
    means = (np.repeat(centres, sizes, axis=0) + spread * rng.standard_normal((M, dim))).astype(np.float32)
    vars_ = np.exp(spread * rng.standard_normal((M, dim))).astype(np.float32)
    weights = np.empty(M, np.float32)
    for j in range(P):
        weights[off[j]:off[j + 1]] = rng.dirichlet(np.full(sizes[j], 2.0))
    return dict(weights=weights, means=means, vars=vars_, pdf_offsets=off, dim=dim)


def repeated(g, mi, iv, off, reps, step=np.float32(-0.01)):
    """The model `reps` times over, repetition r with its gconsts shifted by r * step: each pdf keeps the relative
    scores of its Gaussians (and with them the sensitivity of the base model), while no two repetitions score alike,
    so a tile or a pdf read from the wrong repetition shows."""
    M = len(g)
    shift = np.repeat(np.arange(reps, dtype=np.float32) * step, M)
    offs = np.concatenate([[0]] + [off[1:].astype(np.int64) + r * M for r in range(reps)]).astype(np.int32)
    return (np.tile(g, reps) + shift).astype(np.float32), np.tile(mi, (reps, 1)), np.tile(iv, (reps, 1)), offs


def model_params(am, oracle):
    """(gconsts, means_invvars, inv_vars) as DiagGmm stores them; gconsts by the oracle's ComputeGconsts."""
    inv_vars = (np.float32(1.0) / am["vars"]).astype(np.float32)
    means_invvars = (am["means"] * inv_vars).astype(np.float32)
    g, bad = oracle.gmm_compute_gconsts(am["weights"], means_invvars, inv_vars)
    assert bad == 0
    return g, means_invvars, inv_vars


def frames(rng, T, dim):
    return rng.standard_normal((T, dim)).astype(np.float32)


def dictated_model(score_lists, dim, rng):
    """A model whose pdf j scores exactly score_lists[j] on an all-zero frame: for x = 0 every path computes
    ll = (g + 0) + (-0.5 * 0) = g (fmaf(0, ., 0) adds nothing), and gconsts are an input of the API.
    -> (gconsts, means_invvars, inv_vars, pdf_offsets)."""
    g = np.concatenate([np.asarray(s, np.float32) for s in score_lists])
    M = len(g)
    mi = rng.standard_normal((M, dim)).astype(np.float32)
    iv = np.exp(0.3 * rng.standard_normal((M, dim))).astype(np.float32)
    return g, mi, iv, offsets_of([len(s) for s in score_lists])


MIN_LOG_DIFF = np.float32(math.log(2.0 ** -23))   # kMinLogDiffFloat = Log(FLT_EPSILON), kaldi-math.h:121


def cutoff_of(mx, prune):
    """The float32 cutoff of VectorBase::LogSumExp (kaldi-vector.cc:749-752)."""
    mx = np.asarray(mx, np.float32)
    cutoff = mx + MIN_LOG_DIFF
    if prune > 0.0:
        alt = mx - np.float32(prune)
        cutoff = np.where(alt > cutoff, alt, cutoff)
    return cutoff.astype(np.float32)


def dictated_score_lists(rng):
    """name -> scores of one pdf at the LogSumExp's exact edges (the *prune4* ones are about the cutoff mx - 4).  A single Gaussian at the default cutoff adds FLT_EPSILON to a sum of 1, below any float bound, so 120
    of them stand at the cutoff round the maximum: kept they add 1.4e-5, more than twice the bound."""
    mx = np.float32(0.25)
    at = cutoff_of(mx, -1.0)
    below = np.nextafter(at, np.float32(-np.inf))
    at4 = cutoff_of(mx, 4.0)
    below4 = np.nextafter(at4, np.float32(-np.inf))
    assert at4 == mx - np.float32(4.0) and at == mx + MIN_LOG_DIFF
    d = {
        "at_cutoff_kept": [at] * 60 + [mx] + [at] * 60,
        "below_cutoff_dropped": [below] * 60 + [mx] + [below] * 60,
        "at_prune4_cutoff_kept": [mx, at4],
        "below_prune4_cutoff_dropped": [mx, below4],
        "at_prune4_cutoff_chunk2": [at4] * 9 + [mx] + [below4] * 9,
        "tie_at_max": [-3.5, -1.25, -1.25, -7.0],
        "tie_at_max_across_chunks": [-1.25] + [-9.0] * 20 + [-1.25],
        "equal_128": [-42.5] * 128,
        "single": [-17.0],
        "near_minus_1e4": list(np.float32(-1e4) + np.array([0.0, 0.5, -3.0, 0.25, -12.0, -20.0], np.float32)),
    }
    return {k: np.asarray(v, np.float32) for k, v in d.items()}


# ---------------------------------------------------------------- restated launch decisions
def gemm_path(T, M, env):
    """kh_diag_gmm_loglikes takes the two-GEMM formulation (kh_gmm.hip:494)."""
    return T * M >= GEMM_THRESHOLD and "KH_GMM_NO_GEMM" not in env


def loglikes_dp(D):
    """The LaunchLoglikes<DP> instantiation of the register kernel (kh_gmm.hip:508-512); None: the error of :513."""
    for dp in (16, 32, 40, 64, 96):
        if D <= dp:
            return dp
    return None


def m_per_block(T, M, num_cus):
    """Gaussians per block of the register kernel (LaunchLoglikes, kh_gmm.hip:169-176) -> (m_per_block, grid y).
    More than 64: the kernel's mb loop (:69) takes more than one trip."""
    frame_blocks = -(-T // 256)
    tiles_m = -(-M // KTILE_M)
    my = 1
    while frame_blocks * my < num_cus * 4 and my < tiles_m:
        my *= 2
    my = min(my, tiles_m)
    mpb = -(-tiles_m // my) * KTILE_M
    return mpb, -(-M // mpb)


def tiles(offsets):
    """BuildGmmTiles (kh_gmm.hip:409-423): consecutive whole pdfs, at most 128 Gaussians per tile, as
    (m_begin, m_end, pdf_begin, pdf_end); None when a single pdf has more than 128 Gaussians."""
    off = [int(o) for o in offsets]
    P = len(off) - 1
    out, p = [], 0
    while p < P:
        e = p
        while e < P and off[e + 1] - off[p] <= KGT:
            e += 1
        if e == p:
            return None
        out.append((off[p], off[e], p, e))
        p = e
    return out


def fused_taken(T, D, M, offsets, env):
    """kh_am_gmm_loglikes runs GmmFusedPdfKernel (kh_gmm.hip:550-551, :553)."""
    return (D <= 40 and T * M >= GEMM_THRESHOLD and "KH_GMM_NO_FUSION" not in env and "KH_GMM_NO_GEMM" not in env
            and tiles(offsets) is not None)


def fused_ks(D):
    """The KS of the fused kernel's instantiation (kh_gmm.hip:558-559)."""
    return 8 if D <= 16 else 20


def fused_split(T, n_tiles, num_cus, env):
    """gridDim.y of the fused kernel: the shares of the tile list (LaunchFused, kh_gmm.hip:429-432)."""
    blocks = -(-T // 64)
    split = -(-(16 * 2 * num_cus) // blocks)
    if "KH_GMM_SPLIT" in env:
        split = int(env["KH_GMM_SPLIT"])
    return max(1, min(split, 8, n_tiles))


def share_tiles(n_tiles, split):
    """Tiles per blockIdx.y (kh_gmm.hip:301-302).  LaunchFused cuts the split down to n_tiles (:432), so every share
    holds at least one tile: the kernel's early return for an empty share (ti_begin >= ti_end, :303) cannot be
    reached from the host, whatever KH_GMM_SPLIT says, and no test can execute it."""
    return [n_tiles * (y + 1) // split - n_tiles * y // split for y in range(split)]


def lse_kernel(num_mix):
    """"row": GmmPdfLseRowKernel (the row staged in LDS), "thread": GmmPdfLseKernel (kh_gmm.hip:584)."""
    return "row" if 1024 <= num_mix <= LSE_LDS_FLOATS else "thread"


def slab_rows(M):
    """Frames per slab of the unfused path (kh_gmm.hip:566-568): about 1 GiB of T x M scratch."""
    return max(64, (1 << 28) // ((M + 3) & ~3))


def row_subset(T, extra=(), every=64):
    """Rows for the oracle where the whole matrix would take too long: first, last, both sides of every 64-frame
    boundary (`every` = None: none of them), and both sides of the rows in `extra` (slab boundaries)."""
    rows = {0, T - 1}
    if every:
        for b in range(every, T, every):
            rows.update((b - 1, b))
    for b in extra:
        rows.update(r for r in (b - 2, b - 1, b, b + 1) if 0 <= r < T)
    return np.array(sorted(rows), np.int64)


# ---------------------------------------------------------------- float64 reference and bound
def lse_reference(ll, offsets, prune):
    """(ref, kept): the per-pdf LogSumExp of the float32 per-Gaussian scores ll [T, M].  Maximum, cutoff and the kept
    set f >= cutoff in float32 exactly as kaldi-vector.cc:745-763; the differences, the sum and the log in float64."""
    ll = np.ascontiguousarray(ll, np.float32)
    off = np.asarray(offsets, np.int64)
    sizes = np.diff(off)
    assert off[0] == 0 and off[-1] == ll.shape[1] and (sizes > 0).all()
    mx = np.maximum.reduceat(ll, off[:-1], axis=1)                    # float32
    cutoff = cutoff_of(mx, prune)
    kept = ll >= np.repeat(cutoff, sizes, axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx64 = mx.astype(np.float64)
        term = np.exp(ll.astype(np.float64) - np.repeat(mx64, sizes, axis=1))
        # a dropped Gaussian adds nothing; a kept NaN term (the pdf's scores are all -inf) stays NaN
        term = np.where(kept, term, 0.0)
        ref = mx64 + np.log(np.add.reduceat(term, off[:-1], axis=1))
    return ref, kept


LOG2E = 1.4426950408889634
U = 2.0 ** -24


def lse_c(n):
    """c(n) of the module docstring for pdfs of n Gaussians (array)."""
    n = np.asarray(n, np.float64)
    per_term = 2.0 ** -21 + 15.95 * U + 15.95 * abs(float(np.float32(LOG2E)) / LOG2E - 1.0) + 2.0 ** -23
    log2_ulp = np.spacing(np.log2(n).astype(np.float32)).astype(np.float64) * math.log(2.0)
    prod_ulp = np.spacing(np.log(n).astype(np.float32)).astype(np.float64)
    return per_term + n * 2.0 ** -53 + U + log2_ulp + prod_ulp


def lse_bound(ref, offsets):
    """The elementwise bound 1/2 ulp32(|ref| + 2 c(n)) + 2 c(n) for results [T, P] of pdfs with these offsets."""
    c2 = 2.0 * lse_c(np.diff(np.asarray(offsets, np.int64)))[None, :]
    with np.errstate(invalid="ignore"):
        half_ulp = 0.5 * np.spacing((np.abs(ref) + c2).astype(np.float32)).astype(np.float64)
    return half_ulp + c2


def bound_ratio(got, ref, offsets):
    """max |got - ref| / bound over the finite reference entries; got must be NaN exactly where ref is."""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN where the reference has none (or the reverse)"
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    if not fin.any():
        return 0.0
    return float((np.abs(got - ref)[fin] / lse_bound(ref, offsets)[fin]).max())


# ---------------------------------------------------------------- the models of the GPU module
SLAB_BASE = [130] + EDGE_UNIT * 5 + [306, 270]                        # 4096 Gaussians, three pdfs too large for a tile


# name -> (pdf sizes, dim, seed, repetitions); test_gmm_reference.py checks the reference and the sensitivity on each
def lse_models():
    r = np.random.default_rng(4)
    m = {"edge_d%d" % d: (EDGE_SIZES, d, 100 + d, 1) for d in (13, 16, 17, 39, 40)}
    m["edge_small_d13"] = (EDGE_SIZES_SMALL, 13, 201, 1)
    m["edge_129_d13"] = (EDGE_SIZES_129, 13, 202, 1)
    m["edge_wide_d13"] = (EDGE_SIZES, 13, 203, 33)                    # 134244 Gaussians: T = 33 reaches 1 << 22
    for num_mix, d in ((1023, 41), (1024, 8), (12288, 41), (12289, 8)):
        m["lse_%d" % num_mix] = (uneven_sizes(num_mix, r), d, 300 + d + num_mix, 1)
    m["slab_d8"] = (SLAB_BASE, 8, 400, 64)                            # 262144 Gaussians: slabs of 1024 frames
    return m


def build(name, oracle):
    """(pdf_offsets, gconsts, means_invvars, inv_vars, dim, rng) of a named model; the rng continues into the frames."""
    sizes, dim, seed, reps = lse_models()[name]
    rng = np.random.default_rng(seed)
    am = clustered_model(sizes, dim, rng)
    g, mi, iv = model_params(am, oracle)
    off = am["pdf_offsets"]
    if reps > 1:
        g, mi, iv, off = repeated(g, mi, iv, off, reps)
    return off, g, mi, iv, dim, rng
