"""The <double> instantiation behind the boundary (csrc/kh_double.hip: kh_*_d, and the cudaD_* / cublasDgemm seam of
include/cu_kernels_ansi_hip.h): against the golden vectors of the reference's own CuMatrix<double>
(tests/golden/double_ops.npz) and against the numpy restatement on fresh shapes (odd strides, views, tile edges).
Tolerance: 1e-12 relative (fp64; dgemm / libm vs OCML differ in the last bits), copies and gathers bit-exact."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import double_oracle as D
import dense_dispatch as dd
import double_cases as DC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def gpu_ops(api):
    o = types.SimpleNamespace()

    def add_mat_mat(alpha, A, tA, B, tB, beta, Cm):
        return api.add_mat_mat(dev(Cm), alpha, dev(A), tA, dev(B), tB, beta).cpu().numpy()
    o.add_mat_mat = add_mat_mat
    o.softmax_per_row = lambda x: api.apply_softmax_per_row(torch.empty_like(dev(x)), dev(x)).cpu().numpy()
    o.log_softmax_per_row = lambda x: api.apply_log_softmax_per_row(torch.empty_like(dev(x)), dev(x)).cpu().numpy()
    o.copy_rows = lambda src, idx, rows: api.copy_rows(torch.full((rows, src.shape[1]), 7.0, dtype=torch.float64, device="cuda"),
                                                       dev(src), idx).cpu().numpy()
    o.splice = lambda src, off: api.splice(dev(src), off, torch.empty((src.shape[0], src.shape[1] * len(off)), dtype=torch.float64,
                                                                       device="cuda")).cpu().numpy()
    o.group_pnorm = lambda src, g, p: api.group_pnorm(torch.empty((src.shape[0], src.shape[1] // g), dtype=torch.float64, device="cuda"),
                                                      dev(src), p).cpu().numpy()
    o.add_diag_mat2 = lambda alpha, M, beta, v: api.add_diag_mat2(dev(v), alpha, dev(M), beta).cpu().numpy()
    o.mul_rows_vec = lambda M, v: api.mul_rows_vec(dev(M), dev(v)).cpu().numpy()
    o.mul_cols_vec = lambda M, v: api.mul_cols_vec(dev(M), dev(v)).cpu().numpy()
    o.copy_rows_from_vec = lambda M, v: api.copy_rows_from_vec(dev(M), dev(v)).cpu().numpy()
    o.add_vec_to_rows = lambda M, alpha, v, beta: api.add_vec_to_rows(dev(M), alpha, dev(v), beta).cpu().numpy()
    o.apply_floor = lambda M, f: api.apply_floor(dev(M), f).cpu().numpy()
    o.apply_log = lambda M: api.apply_log(dev(M)).cpu().numpy()
    o.apply_exp = lambda M: api.apply_exp(dev(M)).cpu().numpy()
    o.apply_pow = lambda M, p: api.apply_pow(dev(M), p).cpu().numpy()
    o.scale = lambda M, a: api.scale(dev(M), a).cpu().numpy()
    o.sum_column_ranges = lambda src, r, cols: api.sum_column_ranges(torch.empty((src.shape[0], cols), dtype=torch.float64, device="cuda"),
                                                                     dev(src), r).cpu().numpy()
    o.lookup = lambda M, pairs: api.lookup(dev(M), pairs).cpu().numpy()
    return o


def test_golden_vectors_of_the_reference(api):
    G = load_golden("double_ops")
    ops = gpu_ops(api)
    for name, run, want, tol in DC.cases(G):
        DC.check(name, run(ops), want, tol)


@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (64, 128, 16), (65, 129, 17), (300, 70, 513), (1000, 350, 40)])
def test_add_mat_mat_shapes_strides_and_views(api, m, n, k):
    """Tile edges (64 x 128 x 16 tiles), all transposes, padded strides (Range views), beta over NaN when beta == 0."""
    rng = np.random.default_rng(m * 7 + n)
    for tA in (0, 1):
        for tB in (0, 1):
            A = rng.standard_normal((k, m) if tA else (m, k))
            B = rng.standard_normal((n, k) if tB else (k, n))
            Cm = rng.standard_normal((m, n))
            # operands as views of wider allocations: stride > cols
            Ad = torch.zeros((A.shape[0], A.shape[1] + 3), dtype=torch.float64, device="cuda")[:, :A.shape[1]]
            Bd = torch.zeros((B.shape[0], B.shape[1] + 5), dtype=torch.float64, device="cuda")[:, 2:2 + B.shape[1]]
            Cd = torch.zeros((m, n + 1), dtype=torch.float64, device="cuda")[:, :n]
            Ad.copy_(torch.from_numpy(A)); Bd.copy_(torch.from_numpy(B)); Cd.copy_(torch.from_numpy(Cm))
            api.add_mat_mat(Cd, 0.75, Ad, tA, Bd, tB, -0.5)
            want = D.add_mat_mat(0.75, A, tA, B, tB, -0.5, Cm)
            assert np.abs(Cd.cpu().numpy() - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
            Cd.fill_(float("nan"))
            api.add_mat_mat(Cd, 1.0, Ad, tA, Bd, tB, 0.0)      # beta == 0 overwrites whatever C held
            want = D.add_mat_mat(1.0, A, tA, B, tB, 0.0, Cm)
            assert np.abs(Cd.cpu().numpy() - want).max() <= 1e-11 * max(1.0, np.abs(want).max())


def test_elementwise_on_fresh_shapes(api):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((130, 2049)) * 3.0
    got = api.apply_softmax_per_row(torch.empty((130, 2049), dtype=torch.float64, device="cuda"), dev(x)).cpu().numpy()
    assert np.abs(got - D.softmax_per_row(x)).max() < 1e-14
    assert np.abs(got.sum(1) - 1.0).max() < 1e-13
    got = api.apply_log_softmax_per_row(torch.empty((130, 2049), dtype=torch.float64, device="cuda"), dev(x)).cpu().numpy()
    assert np.abs(got - D.log_softmax_per_row(x)).max() < 1e-12
    src = rng.standard_normal((257, 3500))
    got = api.group_pnorm(torch.empty((257, 350), dtype=torch.float64, device="cuda"), dev(src), 2.0).cpu().numpy()
    assert np.abs(got - D.group_pnorm(src, 10, 2.0)).max() < 1e-12
    idx = rng.integers(-1, 257, 400).astype(np.int32)
    got = api.copy_rows(torch.empty((400, 3500), dtype=torch.float64, device="cuda"), dev(src), idx).cpu().numpy()
    assert np.array_equal(got, D.copy_rows(src, idx, 400))


def test_cudaD_seam_and_cublasDgemm(api):
    """The reference's own launcher names for <double> (cu-kernels-ansi.h) and cublasDgemm (column-major), through ctypes."""
    from importlib import import_module
    lib = import_module("old-kaldi-git_amd.capi").load()

    class MatrixDim(C.Structure):
        _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int32)]

    class Dim3(C.Structure):
        _fields_ = [("x", C.c_uint), ("y", C.c_uint), ("z", C.c_uint)]
    g = Dim3(1, 1, 1)
    rng = np.random.default_rng(11)
    M = rng.standard_normal((33, 70))
    Md = dev(M)
    lib.cudaD_scale.argtypes = [Dim3, Dim3, C.c_void_p, C.c_double, MatrixDim]
    lib.cudaD_scale.restype = None
    lib.cudaD_scale(g, g, Md.data_ptr(), 2.5, MatrixDim(33, 70, 70))
    api.synchronize()
    assert np.array_equal(Md.cpu().numpy(), M * 2.5)
    lib.cudaD_softmax_reduce.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, MatrixDim, C.c_int]
    lib.cudaD_softmax_reduce.restype = None
    y = torch.empty((33, 70), dtype=torch.float64, device="cuda")
    x = dev(M)
    lib.cudaD_softmax_reduce(1, 1, y.data_ptr(), x.data_ptr(), MatrixDim(33, 70, 70), 70)
    api.synchronize()
    assert np.abs(y.cpu().numpy() - D.softmax_per_row(M)).max() < 1e-14
    # cublasDgemm: column-major C (m x n) = alpha op(A) op(B) + beta C
    m, n, k = 19, 23, 31
    A, B, Cm = rng.standard_normal((k, m)), rng.standard_normal((n, k)), rng.standard_normal((n, m))   # row-major views of col-major A (m x k), B (k x n), C (m x n)
    Ad, Bd, Cd = dev(A), dev(B), dev(Cm)
    lib.cublasDgemm.argtypes = [C.c_char, C.c_char, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                C.c_double, C.c_void_p, C.c_int]
    lib.cublasDgemm.restype = None
    lib.cublasDgemm(b"N", b"N", m, n, k, 1.5, Ad.data_ptr(), m, Bd.data_ptr(), k, 0.5, Cd.data_ptr(), m)
    api.synchronize()
    want = 1.5 * (A.T @ B.T) + 0.5 * Cm.T        # column-major result, as an m x n matrix
    assert np.abs(Cd.cpu().numpy().T - want).max() < 1e-12
    assert lib.kh_cuda_seam_status() == 0


# ==================================================================== every branch of kh_double.hip
# The float suite of tests/test_gpu_dense_dispatch.py section by section: every operand is a float64 view into a
# NaN-filled buffer (row padding 1-3, base offset 1) whose padding must still be NaN afterwards, every test first
# asserts the restated launch condition (tests/dense_dispatch.py) of the loop it is about.  References: bit-exact
# numpy / double_oracle for copies, gathers, floor, scale and the vector products; for sums, exp / log / pow and
# norms the oracle at double_cases.RTOL and a numpy long-double restatement (eps 1.08e-19) with a derived bound, or,
# for the transcendental ones, "no further from the long-double value than the oracle is plus a stated number of
# double ulps".
F64 = torch.float64
LD = np.longdouble
U64 = 2.0 ** -53     # unit roundoff of float64
ULP = 2.0 ** -52     # one double ulp, relative (at most)
# Margins above the oracle's own distance from the long-double value, stated before measuring.  One library call
# (exp, log, pow: at most 1 ulp in the device's math library as in the host's): 2 ulps.  A composite of calls, sums
# and a division or root (softmax, log-softmax, the generic p-norm and its rescue): 4 ulps.
ULPS_CALL, ULPS_COMPOSITE = 2, 4


def dmat(host, pad=2, offset=1):
    return dd.mat(host, pad, offset, F64)


def dview(rows, cols, pad=3, offset=1):
    return dd.NanView(rows, cols, cols + pad, offset, dtype=F64)


def dvec(host):
    return dd.vec(host, F64)


def rel_dist(got, truth):
    """Max |got / truth - 1| over the entries whose long-double truth is a normal double; the others (0, or below
    the double range) must be exactly 0 in got."""
    truth = np.asarray(truth, LD)
    got = np.asarray(got, np.float64)
    assert got.shape == truth.shape
    tiny = np.abs(truth) < LD(2.0) ** -1022
    assert np.array_equal(got[tiny], np.zeros(int(tiny.sum())))
    if tiny.all():
        return 0.0
    return float(np.abs(got[~tiny].astype(LD) / truth[~tiny] - 1).max())


def no_further_than_oracle(name, got, want, truth, ulps, dist=rel_dist):
    """The kernel's result is no further from the long-double value than the oracle's is, plus `ulps` double ulps."""
    dk, do = dist(got, truth), dist(want, truth)
    print("%s: max relative distance from long double: kernel %.4g, oracle %.4g" % (name, dk, do))
    assert dk <= do + ulps * ULP, (name, dk, do)


def within_sum_bound(name, got, truth, n, magnitudes):
    """An n-term sum (of products) is within (n + 2) u of the long-double value, times the sum of magnitudes."""
    excess = np.abs(np.asarray(got, np.float64).astype(LD) - truth) - (n + 2) * U64 * np.asarray(magnitudes, LD)
    assert excess.max() <= 0, "%s: bound exceeded by %g" % (name, float(excess.max()))


@pytest.fixture(params=["rows", "cols"])
def shape(request):
    """The two grid-stride shapes of the float suite: more rows than NumCUs()*16 blocks, then more columns than one
    pass of the widest grid (64 blocks of 256)."""
    if request.param == "rows":
        return request.param, (dd.num_cus() * 16 * 4 + 3, 5)
    return request.param, (3, 64 * 256 * 2 + 5)


def assert_map_d_loop(kind, rows, cols):
    """The LaunchMap launch of rows x cols (kh_double.hip:149-160) takes the loop of Map2DD (:144-145) this shape is about."""
    row_loop, col_loop = dd.map_d_strides(rows, cols)
    assert (row_loop, col_loop) == (kind == "rows", kind == "cols"), (rows, cols, row_loop, col_loop)


def inplace_d(fn, host, *args):
    v = dmat(host, 1, 1)
    fn(v.t, *args)
    got = v.host()
    v.assert_padding_untouched()
    return got


def gathers(api, rng, rows, cols, src_rows):
    """copy_rows with indices -1, 0 and last, splice with offsets that clip at both ends: bit-exact."""
    src = rng.standard_normal((src_rows, cols))
    idx = rng.integers(-1, src_rows, rows).astype(np.int32)
    idx[:3] = [src_rows - 1, -1, 0]
    s, out = dmat(src, 3, 1), dview(rows, cols)
    api.copy_rows(out.t, s.t, idx)
    got = out.host()
    out.assert_padding_untouched()
    s.assert_padding_untouched()
    assert np.array_equal(got, D.copy_rows(src, idx, rows))
    assert np.array_equal(got, np.where(idx[:, None] < 0, 0.0, src[np.maximum(idx, 0)]))

    X = rng.standard_normal((rows, cols))
    offsets = np.asarray([-2, 0, 3], np.int32)
    s, out = dmat(X, 1, 1), dview(rows, cols * 3)
    api.splice(s.t, offsets, out.t)
    got = out.host()
    out.assert_padding_untouched()
    s.assert_padding_untouched()
    assert np.array_equal(got, D.splice(X, offsets))
    assert np.array_equal(got[0, :cols], X[0]) and np.array_equal(got[-1, 2 * cols:], X[-1])   # clipped at both ends


def test_gathers_beyond_one_grid_d(api, rng, shape):
    kind, (rows, cols) = shape
    assert_map_d_loop(kind, rows, cols)          # kh_copy_rows_d, kh_double.hip:266
    assert_map_d_loop(kind, rows, cols * 3)      # kh_splice_d launches over d_out, :278
    gathers(api, rng, rows, cols, 101 if kind == "rows" else 7)


def vector_broadcasts(api, rng, rows, cols):
    """copy_rows_from_vec, add_vec_to_rows, mul_rows_vec, mul_cols_vec: one or two roundings per element in the
    kernel's order (alpha v + beta e, no contraction), so bit-exact against numpy."""
    X = rng.standard_normal((rows, cols))
    v, s = rng.standard_normal(cols), rng.standard_normal(rows)
    out = dview(rows, cols)
    api.copy_rows_from_vec(out.t, dvec(v))
    got = out.host()
    out.assert_padding_untouched()
    assert np.array_equal(got, np.broadcast_to(v, (rows, cols)))
    got = inplace_d(lambda M: api.add_vec_to_rows(M, 0.7, dvec(v), 0.3), X)
    assert np.array_equal(got, 0.7 * v[None, :] + 0.3 * X)
    got = inplace_d(lambda M: api.mul_rows_vec(M, dvec(s)), X)
    assert np.array_equal(got, X * s[:, None])
    got = inplace_d(lambda M: api.mul_cols_vec(M, dvec(v)), X)
    assert np.array_equal(got, X * v[None, :])


def test_vector_broadcasts_beyond_one_grid_d(api, rng, shape):
    kind, (rows, cols) = shape
    assert_map_d_loop(kind, rows, cols)
    vector_broadcasts(api, rng, rows, cols)


POWERS = (1.0, 2.0, 0.5, -0.5, 3.3)


def elementwise_maps(api, rng, rows, cols, tag):
    """apply_floor, scale and apply_pow(1 | 2) bit-exact; apply_log, apply_exp and the other powers against the
    oracle at RTOL and no further from long double than the oracle plus ULPS_CALL."""
    X = rng.standard_normal((rows, cols)) * 3.0
    P = rng.random((rows, cols)) * 4.0 + 0.01
    got = inplace_d(lambda M: api.apply_floor(M, -0.2), X)
    assert np.array_equal(got, np.maximum(X, -0.2))
    got = inplace_d(lambda M: api.scale(M, -1.5), X)
    assert np.array_equal(got, X * -1.5)
    for name, fn, want, truth in (("log", api.apply_log, np.log(P), np.log(P.astype(LD))),
                                  ("exp", api.apply_exp, np.exp(X), np.exp(X.astype(LD)))):
        got = inplace_d(fn, P if name == "log" else X)
        DC.check(name, got, want, DC.RTOL)
        no_further_than_oracle("%s apply_%s" % (tag, name), got, want, truth, ULPS_CALL)
    for p in POWERS:
        got = inplace_d(lambda M: api.apply_pow(M, p), P)
        want = D.apply_pow(P, p)
        if p in (1.0, 2.0):
            assert np.array_equal(got, want), p
            continue
        DC.check("pow %g" % p, got, want, DC.RTOL)
        no_further_than_oracle("%s apply_pow %g" % (tag, p), got, want, P.astype(LD) ** LD(p), ULPS_CALL)


def test_elementwise_maps_beyond_one_grid_d(api, rng, shape):
    """Measured on an MI355X, max relative distance from long double (kernel, oracle):
    log 1.215e-16, 1.195e-16; exp 1.318e-16, 1.275e-16; pow 0.5 1.109e-16, 1.109e-16; pow -0.5 2.193e-16, 1.273e-16;
    pow 3.3 2.188e-16, 1.25e-16 (the same at both shapes but for exp at "rows": 1.306e-16)."""
    kind, (rows, cols) = shape
    assert_map_d_loop(kind, rows, cols)
    elementwise_maps(api, rng, rows, cols, kind)


def ld_group_norm(X, group, p):
    g = np.abs(X.astype(LD)).reshape(X.shape[0], -1, group)
    if p == 0.0:
        return (g != 0).sum(2).astype(LD)
    return (g ** LD(p)).sum(2) ** (LD(1.0) / LD(p))


def group_pnorms(api, rng, rows, cols, group, tag):
    """p = 2 and 1: a sum of `group` terms under a root or plain, within (group + 2) u relative of long double (all
    terms positive; the root halves the sum's error and adds its own rounding).  p = 0 counts: exact.  p = 3: the
    generic path, measured against the oracle."""
    X = rng.standard_normal((rows, cols * group))
    X[::2, ::3] = 0.0      # something for p = 0 to skip
    src = dmat(X, 2, 1)
    for p in (2.0, 1.0, 0.0, 3.0):
        out = dview(rows, cols)
        api.group_pnorm(out.t, src.t, p)
        got = out.host()
        out.assert_padding_untouched()
        want, truth = D.group_pnorm(X, group, p), ld_group_norm(X, group, p)
        if p == 0.0:
            assert np.array_equal(got, want) and np.array_equal(got, truth.astype(np.float64))
            continue
        DC.check("group_pnorm %g" % p, got, want, DC.RTOL)
        if p == 3.0:
            no_further_than_oracle("%s group_pnorm 3" % tag, got, want, truth, ULPS_COMPOSITE)
        else:
            within_sum_bound("group_pnorm %g" % p, got, truth, group, truth)
    src.assert_padding_untouched()


def ld_column_ranges(X, pairs):
    x = X.astype(LD)
    truth = np.stack([x[:, b:e].sum(1) for b, e in pairs], 1)
    mags = np.stack([np.abs(x[:, b:e]).sum(1) for b, e in pairs], 1)
    return truth, mags


def column_ranges(api, X, pairs):
    """sum_column_ranges: against the oracle at RTOL; an n-term sum within (n + 2) u of long double times the sum of
    magnitudes; empty ranges exactly 0."""
    rows = X.shape[0]
    ranges = np.asarray(pairs, np.int32).ravel()
    src, out = dmat(X, 2, 1), dview(rows, len(pairs))
    api.sum_column_ranges(out.t, src.t, ranges)
    got = out.host()
    out.assert_padding_untouched()
    src.assert_padding_untouched()
    empty = np.array([b == e for b, e in pairs])
    assert empty.any() and np.array_equal(got[:, empty], np.zeros((rows, int(empty.sum()))))
    assert any(b == 0 and e == X.shape[1] for b, e in pairs)      # one range covers the whole row
    DC.check("sum_column_ranges", got, D.sum_column_ranges(X, ranges, len(pairs)), DC.RTOL)
    truth, mags = ld_column_ranges(X, pairs)
    n = np.asarray([e - b for b, e in pairs], np.float64)[None, :]
    within_sum_bound("sum_column_ranges", got, truth, n, mags)


def test_reductions_beyond_one_grid_d(api, rng, shape):
    """group_pnorm (p = 2, 1, 0, 3) and sum_column_ranges with the OUTPUT at the two grid-stride shapes.
    Measured on an MI355X, p = 3, max relative distance from long double (kernel, oracle):
    rows 4.509e-16, 3.529e-16; cols 6.773e-16, 5.803e-16."""
    kind, (rows, cols) = shape
    assert_map_d_loop(kind, rows, cols)     # both launch over the output: kh_double.hip:291, :339
    group_pnorms(api, rng, rows, cols, 3 if kind == "rows" else 2, kind)
    if kind == "rows":
        X = rng.standard_normal((rows, 7))
        pairs = [(0, 2), (2, 5), (1, 1), (0, 7), (7, 7)]
    else:
        src_cols = 33000
        sizes = rng.multinomial(src_cols, np.full(cols - 1, 1.0 / (cols - 1)))     # about a third of them empty
        ends = np.cumsum(sizes)
        pairs = [(int(b), int(e)) for b, e in zip(ends - sizes, ends)] + [(0, src_cols)]
        X = rng.standard_normal((rows, src_cols))
    assert len(pairs) == cols
    column_ranges(api, X, pairs)


@pytest.mark.parametrize("cols", [37, 255, 256, 257])
def test_block_width_threshold_d(api, rng, cols):
    """LaunchMap picks 64-thread blocks below 256 columns and 256-thread blocks from there on (kh_double.hip:151): 37
    columns (one partial block of 64), 255 (four blocks of 64, the last short), 256 (one full block of 256) and 257
    (two, the second with one column).  Every Map2DD entry point at 9 rows, no grid-stride loop.
    Measured on an MI355X, max relative distance from long double (kernel, oracle):
    the largest over the four widths: log 1.169e-16, 1.092e-16; exp 1.237e-16, 1.042e-16; pow -0.5 1.753e-16, 1.226e-16;
    pow 3.3 2.019e-16, 1.184e-16; group_pnorm 3 2.88e-16, 2.023e-16 (pow 0.5 is a correctly rounded sqrt in both)."""
    rows = 9
    gx, gy, cpp = dd.map_d_grid(rows, cols)
    assert cpp // gx == (256 if cols >= 256 else 64) and dd.map_d_strides(rows, cols) == (False, False)
    assert gx == {37: 1, 255: 4, 256: 1, 257: 2}[cols] and gy == rows
    gathers(api, rng, rows, cols, 11)
    vector_broadcasts(api, rng, rows, cols)
    elementwise_maps(api, rng, rows, cols, "cols %d" % cols)
    group_pnorms(api, rng, rows, cols, 5, "cols %d" % cols)
    column_ranges(api, rng.standard_normal((rows, cols + 3)),
                  [(0, 0), (0, cols + 3)] + [(j, j + 1 + j % 4) for j in range(cols - 2)])


# ---------------------------------------------------------------- softmax, log-softmax
def softmax_input(rng, rows, cols):
    """Rows in order: random, all equal, with -inf entries, a spread of 1400 (exp underflows to 0 for all but the
    maximum; the log-softmax of the minimum stays finite), random."""
    X = rng.standard_normal((rows, cols)) * 3.0
    if rows > 1:
        X[1] = 0.375
    if rows > 2 and cols > 1:
        X[2, ::2] = -np.inf
        X[2, cols // 2 | 1] = 1.5       # an odd column: at least one finite entry
    if rows > 3 and cols > 1:
        X[3] = -700.0
        X[3, cols // 3] = 700.0
    return X


def ld_softmax(X):
    x = X.astype(LD)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def ld_log_softmax(X):
    x = X.astype(LD)
    z = x - x.max(1, keepdims=True)
    return z - np.log(np.exp(z).sum(1, keepdims=True))


def log_dist(got, truth):
    """Distance of a log-softmax from long double relative to max(|value|, 1) (a value near 0 is a difference of
    O(1) numbers); -inf must be -inf."""
    inf = np.isinf(truth)
    assert np.array_equal(np.asarray(got)[inf], np.asarray(truth, np.float64)[inf])
    if inf.all():
        return 0.0
    g, t = np.asarray(got, np.float64)[~inf].astype(LD), truth[~inf]
    return float((np.abs(g - t) / np.maximum(np.abs(t), 1)).max())


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 130])
def test_softmax_one_wave_per_row_d(api, rng, cols):
    """SoftmaxDKernel (kh_double.hip:118-139): one wave per row and four per block, so rows 1, 3, 4, 5 lie either side
    of a block; columns either side of one and two passes of the lane loop; x_stride != y_stride; and in place
    (y == x, the guarantee stated in include/kaldi_hip.h).  Rows of equal values, with -inf entries and with a spread
    of 1400.  Against the oracle at RTOL, rows sum to 1 within (cols + 2) u, and no further from long double than the
    oracle plus ULPS_COMPOSITE.
    Measured on an MI355X, max distance from long double over rows and both modes (kernel, oracle):
    cols 63: softmax 1.051e-15, 1.101e-15, log-softmax 1.992e-16, 1.682e-16; cols 64: 1.192e-15, 9.676e-16 and 1.963e-16,
    1.188e-16; cols 65: 1.179e-15, 1.039e-15 and 2.08e-16, 3.32e-16; cols 130: 1.956e-15, 1.841e-15 and 2.113e-16, 1.919e-16;
    cols 1: 0 everywhere.  (Both share the rounding of x - max, which exp turns into |x - max| u.)"""
    worst = {}
    for rows in (1, 3, 4, 5):
        X = softmax_input(rng, rows, cols)
        if rows >= 4 and cols > 1:
            with np.errstate(under="ignore"):
                assert (np.exp(X[3] - X[3].max()) == 0).sum() == cols - 1      # exp underflows for all but the maximum
        for log in (False, True):
            fn = api.apply_log_softmax_per_row if log else api.apply_softmax_per_row
            with np.errstate(under="ignore", divide="ignore"):
                want = (D.log_softmax_per_row if log else D.softmax_per_row)(X)
                truth = (ld_log_softmax if log else ld_softmax)(X)
            for in_place in (False, True):
                x = dmat(X, 2, 1)
                y = x if in_place else dview(rows, cols, 3, 1)
                assert in_place or rows == 1 or x.t.stride(0) != y.t.stride(0)
                fn(y.t, x.t)
                got = y.host()
                y.assert_padding_untouched()
                x.assert_padding_untouched()
                if not in_place:
                    assert np.array_equal(x.host(), X)
                fin = np.isfinite(want)
                assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
                DC.check("softmax", got[fin], want[fin], DC.RTOL)
                if log:
                    assert np.isfinite(got[X > -np.inf]).all()          # the minimum of the spread row included
                    dk, do = log_dist(got, truth), log_dist(want, truth)
                else:
                    assert np.abs(got.astype(LD).sum(1) - 1).max() <= (cols + 2) * U64
                    dk, do = rel_dist(got, truth), rel_dist(want, truth)
                assert dk <= do + ULPS_COMPOSITE * ULP, (rows, log, in_place, dk, do)
                k = "log-softmax" if log else "softmax"
                worst[k] = max(worst.get(k, (0.0, 0.0)), (dk, do))
    for k, (dk, do) in sorted(worst.items()):
        print("cols %d %s: max distance from long double: kernel %.4g, oracle %.4g" % (cols, k, dk, do))


# ---------------------------------------------------------------- group_pnorm's overflow rescue
def test_group_pnorm_overflow_rescue_d(api, rng):
    """GroupNorm's rescue (kh_double.hip:186-195): one group of one row near 1e120 under p = 3, whose cubes overflow
    double, is rescaled by its largest magnitude; the other groups and rows take the plain path; p = 0.5 on the same
    input does not overflow; a group of zeros under generic p is exactly 0.
    Measured on an MI355X, max relative distance from long double (kernel, oracle):
    p = 3: all groups 1.949e-16, 1.441e-16, the rescued group 8.191e-17, 8.132e-17; p = 0.5: 3.866e-16, 3.866e-16 and
    5.909e-17, 5.909e-17."""
    group = 5
    X = rng.standard_normal((3, 4 * group))
    X[0, :group] = 1e120 * (1.0 + 0.1 * rng.standard_normal(group))
    X[1, group:2 * group] = 0.0
    with np.errstate(over="ignore"):
        plain = (np.abs(X.reshape(3, 4, group)) ** 3.0).sum(2)
    assert np.isinf(plain[0, 0]) and np.isfinite(np.delete(plain.ravel(), 0)).all()    # only that group overflows
    want3 = D.group_pnorm(X, group, 3.0)
    assert np.isfinite(want3).all() and want3[0, 0] > 1e120
    src = dmat(X, 2, 1)
    for p, want in ((3.0, want3), (0.5, D.group_pnorm(X, group, 0.5))):
        out = dview(3, 4)
        api.group_pnorm(out.t, src.t, p)
        got = out.host()
        out.assert_padding_untouched()
        assert np.isfinite(got).all() and got[1, 1] == 0.0
        DC.check("group_pnorm %g" % p, got, want, DC.RTOL)
        truth = ld_group_norm(X, group, p)
        assert np.isfinite(truth.astype(np.float64)).all()
        no_further_than_oracle("rescue input, p = %g" % p, got, want, truth, ULPS_COMPOSITE)
        no_further_than_oracle("rescue input, p = %g, the 1e120 group" % p, got[:1, :1], want[:1, :1], truth[:1, :1], ULPS_COMPOSITE)
    src.assert_padding_untouched()


# ---------------------------------------------------------------- add_diag_mat2, lookup
@pytest.mark.parametrize("cols", [1, 64, 65, 200])
def test_add_diag_mat2_row_loop_d(api, rng, cols):
    """AddDiagMat2DKernel with more rows than wave slots (kh_double.hip:201, :301); columns either side of one pass of
    the lane loop; beta = 0 over a NaN-filled v, which must not be read.  v is a padded view too.  cols products and
    their sum, alpha times it, beta v, their sum: within (cols + 2) u of long double times the sum of magnitudes."""
    rows = dd.num_cus() * 8 * 4 + 3
    assert dd.add_diag_mat2_d_row_loop(rows) and not dd.add_diag_mat2_d_row_loop(rows - 3)
    X = rng.standard_normal((rows, cols))
    v0 = rng.standard_normal(rows)
    src = dmat(X, 3, 1)
    x = X.astype(LD)
    sq = (x * x).sum(1)
    for alpha, beta in ((0.7, 0.3), (0.7, 0.0)):
        v = dd.NanView(1, rows, rows + 2, 1, None if beta == 0.0 else v0[None, :], F64)
        api.add_diag_mat2(v.t[0], alpha, src.t, beta)
        got = v.host()[0]
        v.assert_padding_untouched()
        assert np.isfinite(got).all()
        vin = v0 if beta != 0.0 else np.zeros(rows)
        DC.check("add_diag_mat2", got, D.add_diag_mat2(alpha, X, beta, vin), DC.RTOL)
        within_sum_bound("add_diag_mat2", got, LD(alpha) * sq + LD(beta) * vin, cols, abs(alpha) * sq + np.abs(beta * vin))
    src.assert_padding_untouched()


def test_lookup_loop_and_edges_d(api, rng):
    """LookupDKernel with more pairs than threads (kh_double.hip:213, :353), no pairs at all, and pairs on the last
    row and the last column of a padded view.  Bit-exact."""
    X = rng.standard_normal((37, 53))
    M = dmat(X, 3, 1)
    n = dd.num_cus() * 8 * 256 + 7
    assert dd.lookup_d_loop(n) and not dd.lookup_d_loop(n - 7) and not dd.lookup_d_loop(5)
    pairs = np.stack([rng.integers(0, 37, n), rng.integers(0, 53, n)], 1).astype(np.int32)
    pairs[:3] = [(36, 52), (36, 0), (0, 52)]
    pairs[-1] = (36, 52)
    got = api.lookup(M.t, pairs.ravel()).cpu().numpy()
    assert np.array_equal(got, X[pairs[:, 0], pairs[:, 1]]) and np.array_equal(got, D.lookup(X, pairs.ravel()))
    edge = np.asarray([(36, c) for c in range(53)] + [(r, 52) for r in range(37)], np.int32)
    got = api.lookup(M.t, edge.ravel()).cpu().numpy()
    assert np.array_equal(got, np.concatenate([X[36], X[:, 52]]))
    assert api.lookup(M.t, np.zeros(0, np.int32)).numel() == 0
    api.synchronize()
    M.assert_padding_untouched()
    assert np.array_equal(M.host(), X)
