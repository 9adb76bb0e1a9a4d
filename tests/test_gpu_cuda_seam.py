"""GPU: the reference's lower C-ABI seam (include/cu_kernels_ansi_hip.h) — the
cu-kernels-ansi.h launcher names called the way cu-matrix.cc calls them (geometry
arguments by value, MatrixDim by value), checked against the CPU oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cases
import dense_dispatch as dd
import double_cases as DC
from oracle import double_oracle as D

pytestmark = pytest.mark.gpu


class Dim3(C.Structure):
    _fields_ = [("x", C.c_uint), ("y", C.c_uint), ("z", C.c_uint)]


class MatrixDim(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int32)]


G, B = Dim3(1, 1, 1), Dim3(16, 16, 1)   # ignored by the library
vp, f32, i32 = C.c_void_p, C.c_float, C.c_int


# The signatures of include/cu_kernels_ansi_hip.h, written once for float; the cudaD_* / cublasDgemm twins are the same
# with double where float stands.
SIG_F = {
    "cudaF_softmax_reduce": [C.c_size_t, C.c_size_t, vp, vp, MatrixDim, i32],
    "cudaF_log_softmax_reduce": [C.c_size_t, C.c_size_t, vp, vp, MatrixDim, i32],
    "cudaF_copy_rows": [Dim3, Dim3, vp, vp, vp, MatrixDim, i32],
    "cudaF_splice": [Dim3, Dim3, vp, vp, vp, MatrixDim, MatrixDim],
    "cudaF_group_pnorm": [Dim3, Dim3, vp, vp, MatrixDim, i32, i32, f32],
    "cudaF_add_diag_mat_mat": [i32, i32, f32, vp, i32, vp, i32, i32, i32, vp, i32, i32, i32, f32],
    "cudaF_mul_cols_vec": [Dim3, Dim3, vp, vp, MatrixDim],
    "cudaF_mul_rows_vec": [Dim3, Dim3, vp, vp, MatrixDim],
    "cudaF_copy_rows_from_vec": [Dim3, Dim3, vp, MatrixDim, vp],
    "cudaF_add_vec_to_rows": [Dim3, Dim3, f32, vp, f32, vp, MatrixDim],
    "cudaF_apply_exp": [Dim3, Dim3, vp, MatrixDim],
    "cudaF_apply_pow": [Dim3, Dim3, vp, f32, MatrixDim],
    "cudaF_apply_floor": [Dim3, Dim3, vp, f32, MatrixDim],
    "cudaF_scale": [Dim3, Dim3, vp, f32, MatrixDim],
    "cudaF_apply_log": [Dim3, Dim3, vp, MatrixDim],
    "cudaF_sum_column_ranges": [Dim3, Dim3, vp, MatrixDim, vp, MatrixDim, vp],
    "cudaF_matrix_lookup": [Dim3, Dim3, vp, MatrixDim, vp, i32, vp],
    "cudaF_comp_obj_deriv": [Dim3, Dim3, vp, i32, vp, MatrixDim, vp, MatrixDim, vp],
    "cublasSgemm": [C.c_char, C.c_char, i32, i32, i32, f32, vp, i32, vp, i32, f32, vp, i32],
}


def double_twin(name, args):
    name = "cublasDgemm" if name == "cublasSgemm" else name.replace("cudaF_", "cudaD_")
    return name, [C.c_double if a is f32 else a for a in args]


SIG = dict(SIG_F)
SIG.update(double_twin(name, args) for name, args in SIG_F.items())


@pytest.fixture(scope="module")
def seam(api):
    import torch
    lib = C.CDLL(api.capi.LIB_PATH)
    sig = SIG
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, None
    lib.kh_cuda_seam_status.restype = C.c_int

    class S:
        pass
    s = S()
    s.lib, s.torch, s.api = lib, torch, api

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s.dev = dev
    s.ptr = lambda t: vp(t.data_ptr())
    s.dim = lambda t: MatrixDim(t.shape[0], t.shape[1], t.stride(0))

    def host(t):
        api.synchronize()
        assert lib.kh_cuda_seam_status() == 0, api.lib().kh_last_error()
        return t.cpu().numpy()
    s.host = host
    return s


def test_softmax_pnorm_copy_rows_splice(seam, oracle, rng):
    s = seam
    X = (rng.standard_normal((37, 300)) * 3).astype(np.float32)
    x = s.dev(X)
    y = s.torch.empty_like(x)
    s.lib.cudaF_softmax_reduce(1, 256, s.ptr(y), s.ptr(x), s.dim(y), x.stride(0))
    cases.close(s.host(y), oracle.softmax_per_row(X), rtol=1e-5, atol=1e-30)
    s.lib.cudaF_log_softmax_reduce(1, 256, s.ptr(y), s.ptr(x), s.dim(y), x.stride(0))
    cases.close(s.host(y), oracle.log_softmax_per_row(X), rtol=1e-5, atol=5e-5)
    yp = s.torch.empty((37, 30), device="cuda")
    s.lib.cudaF_group_pnorm(G, B, s.ptr(yp), s.ptr(x), s.dim(yp), x.stride(0), 10, 2.0)
    cases.close(s.host(yp), oracle.group_pnorm(X, 10, 2.0))
    idx = rng.integers(-1, 37, 50).astype(np.int32)
    yc = s.torch.empty((50, 300), device="cuda")
    s.lib.cudaF_copy_rows(G, B, s.ptr(yc), s.ptr(x), s.ptr(s.dev(idx)), s.dim(yc), x.stride(0))
    cases.exact(s.host(yc), oracle.copy_rows(X, idx))
    off = np.asarray([-2, 0, 3], np.int32)
    ys = s.torch.empty((37, 900), device="cuda")
    s.lib.cudaF_splice(G, B, s.ptr(ys), s.ptr(x), s.ptr(s.dev(off)), s.dim(ys), s.dim(x))
    cases.exact(s.host(ys), oracle.splice(X, off))


def test_elementwise_and_broadcasts(seam, rng):
    s = seam
    X = (np.abs(rng.standard_normal((23, 70))) + 0.1).astype(np.float32)
    v_r = rng.standard_normal(23).astype(np.float32)
    v_c = rng.standard_normal(70).astype(np.float32)
    m = s.dev(X); s.lib.cudaF_apply_log(G, B, s.ptr(m), s.dim(m))
    cases.close(s.host(m), np.log(X), rtol=2e-6, atol=1e-6)
    m = s.dev(X); s.lib.cudaF_apply_exp(G, B, s.ptr(m), s.dim(m))
    cases.close(s.host(m), np.exp(X), rtol=2e-6)
    m = s.dev(X); s.lib.cudaF_apply_pow(G, B, s.ptr(m), 0.5, s.dim(m))
    cases.close(s.host(m), np.sqrt(X), rtol=2e-6)
    m = s.dev(X); s.lib.cudaF_apply_floor(G, B, s.ptr(m), 0.7, s.dim(m))
    cases.exact(s.host(m), np.maximum(X, np.float32(0.7)))
    m = s.dev(X); s.lib.cudaF_scale(G, B, s.ptr(m), 0.25, s.dim(m))
    cases.exact(s.host(m), X * np.float32(0.25))
    m = s.dev(X); s.lib.cudaF_mul_rows_vec(G, B, s.ptr(m), s.ptr(s.dev(v_r)), s.dim(m))
    cases.exact(s.host(m), X * v_r[:, None])
    m = s.dev(X); s.lib.cudaF_mul_cols_vec(G, B, s.ptr(m), s.ptr(s.dev(v_c)), s.dim(m))
    cases.exact(s.host(m), X * v_c[None, :])
    m = s.dev(X); s.lib.cudaF_copy_rows_from_vec(G, B, s.ptr(m), s.dim(m), s.ptr(s.dev(v_c)))
    cases.exact(s.host(m), np.broadcast_to(v_c, X.shape))
    m = s.dev(X); s.lib.cudaF_add_vec_to_rows(G, B, 2.0, s.ptr(s.dev(v_c)), 1.0, s.ptr(m), s.dim(m))
    cases.exact(s.host(m), np.float32(2.0) * v_c[None, :] + X)


def test_ranges_lookup_objf_diag(seam, oracle, rng):
    s = seam
    X = rng.standard_normal((19, 120)).astype(np.float32)
    x = s.dev(X)
    sizes = 1 + rng.multinomial(120 - 40, np.full(40, 1 / 40))
    ends = np.cumsum(sizes)
    ranges = np.stack([ends - sizes, ends], 1).astype(np.int32)
    y = s.torch.empty((19, 40), device="cuda")
    s.lib.cudaF_sum_column_ranges(G, B, s.ptr(y), s.dim(y), s.ptr(x), s.dim(x), s.ptr(s.dev(ranges)))
    cases.close(s.host(y), oracle.sum_column_ranges(X, ranges.ravel()), atol=1e-5)
    pairs = np.stack([rng.integers(0, 19, 33), rng.integers(0, 120, 33)], 1).astype(np.int32)
    out = s.torch.empty(33, device="cuda")
    s.lib.cudaF_matrix_lookup(G, B, s.ptr(x), s.dim(x), s.ptr(s.dev(pairs)), 33, s.ptr(out))
    cases.exact(s.host(out), X[pairs[:, 0], pairs[:, 1]])
    # CompObjfAndDeriv: MatrixElement<float> array on the device, t = 2 floats on the device
    P = (np.abs(rng.standard_normal((19, 120))) + 0.05).astype(np.float32)
    el = np.zeros(25, dtype=[("row", np.int32), ("column", np.int32), ("weight", np.float32)])
    el["row"], el["column"] = rng.permutation(19 * 120)[:25] // 120, rng.permutation(120)[:25]
    el["weight"] = rng.uniform(0.2, 1.5, 25).astype(np.float32)
    d_el = s.torch.from_numpy(el.view(np.uint8).copy()).cuda()
    p, deriv, t = s.dev(P), s.torch.zeros((19, 120), device="cuda"), s.torch.empty(2, device="cuda")
    s.lib.cudaF_comp_obj_deriv(G, B, s.ptr(d_el), 25, s.ptr(p), s.dim(p), s.ptr(deriv), s.dim(deriv), s.ptr(t))
    want_d = np.zeros_like(P)
    np.add.at(want_d, (el["row"], el["column"]), el["weight"] / P[el["row"], el["column"]])
    cases.close(s.host(deriv), want_d, rtol=1e-6)
    tt = s.host(t)
    assert abs(tt[0] - float(np.sum(el["weight"].astype(np.float64) * np.log(P[el["row"], el["column"]].astype(np.float64))))) < 1e-4
    assert abs(tt[1] - float(el["weight"].astype(np.float64).sum())) < 1e-5
    # AddDiagMat2 (N = M^T) and the general strided AddDiagMatMat
    M = rng.standard_normal((19, 120)).astype(np.float32)
    N = rng.standard_normal((120, 19)).astype(np.float32)
    m, n = s.dev(M), s.dev(N)
    v = s.dev(np.ones(19, np.float32))
    s.lib.cudaF_add_diag_mat_mat(1, 256, 0.5, s.ptr(v), 19, s.ptr(m), 120, 120, 1, s.ptr(m), 1, 120, 1, 2.0)
    cases.close(s.host(v), 2.0 + 0.5 * (M.astype(np.float64) ** 2).sum(1), rtol=1e-5)
    v = s.dev(np.ones(19, np.float32))
    s.lib.cudaF_add_diag_mat_mat(1, 256, 1.0, s.ptr(v), 19, s.ptr(m), 120, 120, 1, s.ptr(n), 19, 1, 1, 0.0)
    cases.close(s.host(v), np.einsum("ij,ji->i", M.astype(np.float64), N.astype(np.float64)), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_cublas_sgemm_as_cu_matrix_calls_it(seam, oracle, rng, tA, tB):
    """CuMatrixBase::AddMatMat (cu-matrix.cc:947-982) hands the ROW-major operands to the
    column-major BLAS swapped: cublas_gemm(transB, transA, m = C.cols, n = C.rows, k, alpha,
    B, B.stride, A, A.stride, beta, C, C.stride)."""
    s = seam
    mm, nn, kk = 45, 70, 33
    A = rng.standard_normal((kk, mm) if tA else (mm, kk)).astype(np.float32)
    Bm = rng.standard_normal((nn, kk) if tB else (kk, nn)).astype(np.float32)
    C0 = rng.standard_normal((mm, nn)).astype(np.float32)
    a, b, c = s.dev(A), s.dev(Bm), s.dev(C0)
    s.lib.cublasSgemm(b"T" if tB else b"N", b"T" if tA else b"N", nn, mm, kk, 0.5, s.ptr(b), b.stride(0),
                      s.ptr(a), a.stride(0), 0.25, s.ptr(c), c.stride(0))
    cases.exact(s.host(c), oracle.add_mat_mat(0.5, A, tA, Bm, tB, 0.25, C0))


def test_errors_are_recorded(seam):
    s = seam
    s.lib.cudaF_apply_log(G, B, None, MatrixDim(3, 3, 2))   # stride < cols
    assert s.lib.kh_cuda_seam_status() != 0
    assert s.lib.kh_cuda_seam_status() == 0


# ==================================================================== every launcher, both types, on sub-matrix views
# Each launcher called the way cu-matrix.cc / cu-vector.cc / cu-math.cc call it on CuSubMatrix operands: stride > cols,
# an offset base and, wherever the signature has two strides, two different ones.  The views lie in NaN-filled
# buffers (tests/dense_dispatch.py): a launcher that hands the wrong stride on reads NaN or writes padding.
LD = np.longdouble
U64 = 2.0 ** -53
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cu_kernels_ansi_hip.h")
C_TYPES = {"size_t": C.c_size_t, "KhDim3": Dim3, "MatrixDim": MatrixDim, "int": i32, "int32_t": i32, "float": f32,
           "double": C.c_double, "char": C.c_char}

# launcher (without cudaF_ / cudaD_; "gemm" = cublasSgemm / cublasDgemm) -> the test below that calls it for both types
COVERED = {
    "softmax_reduce": "test_softmax_launchers_on_col_ranges",
    "log_softmax_reduce": "test_softmax_launchers_on_col_ranges",
    "copy_rows": "test_gather_and_pnorm_launchers",
    "splice": "test_gather_and_pnorm_launchers",
    "group_pnorm": "test_gather_and_pnorm_launchers",
    "mul_cols_vec": "test_vector_launchers",
    "mul_rows_vec": "test_vector_launchers",
    "copy_rows_from_vec": "test_vector_launchers",
    "add_vec_to_rows": "test_vector_launchers",
    "apply_exp": "test_elementwise_launchers",
    "apply_pow": "test_elementwise_launchers",
    "apply_floor": "test_elementwise_launchers",
    "scale": "test_elementwise_launchers",
    "apply_log": "test_elementwise_launchers",
    "sum_column_ranges": "test_range_and_lookup_launchers",
    "matrix_lookup": "test_range_and_lookup_launchers",
    "add_diag_mat_mat": "test_add_diag_mat_mat_forms",
    "comp_obj_deriv": "test_comp_obj_deriv",
    "gemm": "test_gemm_as_add_mat_mat_issues_it",
}


def header_prototypes():
    """name -> ctypes argument list of every launcher prototype of include/cu_kernels_ansi_hip.h."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for name, params in re.findall(r"\bvoid\s+(cuda[A-Z]_\w+|cublas\w+)\s*\(([^)]*)\)\s*;", text):
        protos[name] = [vp if "*" in prm else C_TYPES[prm.replace("const", "").split()[0]] for prm in params.split(",")]
    return protos


def test_every_prototype_of_the_header_has_a_signature_and_a_test():
    """List-driven: the header's prototypes are exactly the signature table, argument for argument, and each is
    assigned to a test of this module that exists (the `call` fixture fails a test that does not call what it is
    assigned).  A launcher added to the header without a test fails here."""
    protos = header_prototypes()
    assert len(protos) == 38 and set(protos) == set(SIG), sorted(set(protos) ^ set(SIG))
    for name, args in protos.items():
        assert args == SIG[name], name
    bases = {"gemm" if n.startswith("cublas") else n.split("_", 1)[1] for n in protos}
    assert bases == set(COVERED), sorted(bases ^ set(COVERED))
    for base, test in COVERED.items():
        assert callable(globals().get(test)), (base, test)


class Real:
    def __init__(self, name):
        import torch
        self.double = name == "float64"
        self.torch = getattr(torch, name)
        self.np = np.float64 if self.double else np.float32
        self.prefix = "cudaD_" if self.double else "cudaF_"
        self.gemm = "cublasDgemm" if self.double else "cublasSgemm"
        self.u = 2.0 ** (-53 if self.double else -24)

    def mat(self, host, pad, offset=1):
        return dd.mat(np.asarray(host, self.np), pad, offset, self.torch)

    def blank(self, rows, cols, pad, offset=1):
        return dd.NanView(rows, cols, cols + pad, offset, dtype=self.torch)

    def vec(self, host):
        return dd.vec(np.asarray(host, self.np), self.torch)

    def approx(self, name, got, want, rtol=cases.RTOL, atol=cases.ATOL):
        """The project's tolerance for an op that is not bit-exact: double_cases.RTOL for double, cases.close for float."""
        if self.double:
            DC.check(name, got, want, DC.RTOL)
        else:
            cases.close(got, want, rtol=rtol, atol=atol)


@pytest.fixture(params=["float32", "float64"])
def real(request):
    return Real(request.param)


@pytest.fixture
def call(request, seam, real):
    """call(launcher, *args) for this test's element type; afterwards the test must have called every launcher that
    COVERED assigns to it."""
    called = set()

    def call(base, *args):
        called.add(base)
        getattr(seam.lib, real.gemm if base == "gemm" else real.prefix + base)(*args)
    yield call
    mine = {b for b, t in COVERED.items() if t == request.node.originalname}
    assert mine <= called, "not called: %s" % sorted(mine - called)


def dim(v):
    return MatrixDim(v.shape[0], v.shape[1], v.stride)


def ptr(v):
    return vp((v.t if isinstance(v, dd.NanView) else v).data_ptr())


def done(seam, *views):
    """Wait, require a clean status and untouched padding of every view."""
    seam.api.synchronize()
    assert seam.lib.kh_cuda_seam_status() == 0, seam.api.lib().kh_last_error()
    for v in views:
        v.assert_padding_untouched()


def i32dev(seam, a):
    return seam.torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def softmax64(X, log):
    x = X.astype(np.float64)
    z = x - x.max(1, keepdims=True)
    return z - np.log(np.exp(z).sum(1, keepdims=True)) if log else np.exp(z) / np.exp(z).sum(1, keepdims=True)


def test_softmax_launchers_on_col_ranges(seam, call, real, rng):
    """The ColRange pair of nnet-activation.h:112-115: columns 11..80 of a 90-wide input, columns 5..74 of an 84-wide
    output, so src_stride (90) > d.stride (84) > cols (70)."""
    X = (rng.standard_normal((23, 70)) * 3).astype(real.np)
    x, y = dd.NanView(23, 70, 90, 11, X, real.torch), dd.NanView(23, 70, 84, 5, dtype=real.torch)
    assert x.stride > y.stride > 70
    call("softmax_reduce", 1, 256, ptr(y), ptr(x), dim(y), x.stride)
    done(seam, x, y)
    real.approx("softmax", y.host(), softmax64(X, False), rtol=1e-5, atol=1e-30)
    call("log_softmax_reduce", 1, 256, ptr(y), ptr(x), dim(y), x.stride)
    done(seam, x, y)
    real.approx("log-softmax", y.host(), softmax64(X, True), rtol=1e-5, atol=5e-5)
    cases.exact(x.host(), X)


def test_gather_and_pnorm_launchers(seam, call, real, rng):
    """copy_rows(dst, src, reorder, dst_dim, src_stride), splice(y, x, off, d_out, d_in) with the number of offsets
    derived from the two widths, group_pnorm(y, x, d, src_stride, group_size, power)."""
    X = rng.standard_normal((23, 70)).astype(real.np)
    x = real.mat(X, 5, 2)
    idx = rng.integers(-1, 23, 31).astype(np.int32)
    idx[:3] = [22, -1, 0]
    y = real.blank(31, 70, 2)
    assert x.stride != y.stride
    call("copy_rows", G, B, ptr(y), ptr(x), ptr(i32dev(seam, idx)), dim(y), x.stride)
    done(seam, x, y)
    cases.exact(y.host(), D.copy_rows(X, idx, 31).astype(real.np))
    off = np.asarray([-2, 0, 3], np.int32)
    y = real.blank(23, 210, 1)
    assert x.stride != y.stride and y.shape[1] // x.shape[1] == 3
    call("splice", G, B, ptr(y), ptr(x), ptr(i32dev(seam, off)), dim(y), dim(x))
    done(seam, x, y)
    cases.exact(y.host(), D.splice(X, off))
    y = real.blank(23, 7, 2)
    call("group_pnorm", G, B, ptr(y), ptr(x), dim(y), x.stride, 10, 2.0)
    done(seam, x, y)
    real.approx("group_pnorm", y.host(), D.group_pnorm(X.astype(np.float64), 10, 2.0))
    cases.exact(x.host(), X)


def test_vector_launchers(seam, call, real, rng):
    """mul_cols_vec / mul_rows_vec (mat, scale, d), copy_rows_from_vec (mat_out, d_out, v_in), add_vec_to_rows (alpha,
    row, beta, dst, d) with alpha != beta.  One or two roundings per element, no contraction: bit-exact."""
    X = rng.standard_normal((23, 70)).astype(real.np)
    v_r, v_c = rng.standard_normal(23).astype(real.np), rng.standard_normal(70).astype(real.np)
    m = real.mat(X, 3, 2)
    call("mul_cols_vec", G, B, ptr(m), ptr(real.vec(v_c)), dim(m))
    done(seam, m)
    cases.exact(m.host(), X * v_c[None, :])
    m = real.mat(X, 3, 2)
    call("mul_rows_vec", G, B, ptr(m), ptr(real.vec(v_r)), dim(m))
    done(seam, m)
    cases.exact(m.host(), X * v_r[:, None])
    m = real.blank(23, 70, 3, 2)
    call("copy_rows_from_vec", G, B, ptr(m), dim(m), ptr(real.vec(v_c)))
    done(seam, m)
    cases.exact(m.host(), np.broadcast_to(v_c, X.shape))
    m = real.mat(X, 3, 2)
    call("add_vec_to_rows", G, B, 0.75, ptr(real.vec(v_c)), 0.3, ptr(m), dim(m))
    done(seam, m)
    cases.exact(m.host(), real.np(0.75) * v_c[None, :] + real.np(0.3) * X)


def test_elementwise_launchers(seam, call, real, rng):
    """apply_exp / apply_log (mat, d) and apply_pow / apply_floor / scale (mat, value, d) on a 23 x 70 view of stride 73."""
    X = (np.abs(rng.standard_normal((23, 70))) + 0.1).astype(real.np)
    x64 = X.astype(np.float64)
    for name, args, want, exact in (("apply_exp", (), np.exp(x64), False), ("apply_log", (), np.log(x64), False),
                                    ("apply_pow", (0.5,), np.sqrt(x64), False), ("apply_pow", (3.3,), x64 ** 3.3, False),
                                    ("apply_floor", (0.7,), np.maximum(X, real.np(0.7)), True),
                                    ("scale", (0.3,), X * real.np(0.3), True)):
        m = real.mat(X, 3, 2)
        call(name, G, B, ptr(m), *(args + (dim(m),)))
        done(seam, m)
        if exact:
            cases.exact(m.host(), want)
        else:
            real.approx(name, m.host(), want, rtol=2e-6, atol=1e-6)


def sizes_of(pairs):
    return (pairs["second"] - pairs["first"]).astype(np.float64)[None, :]


def test_range_and_lookup_launchers(seam, call, real, rng):
    """sum_column_ranges (data, dim, src_data, src_dim, Int32Pair *) with dim.stride != src_dim.stride, some empty
    ranges and one over the whole row; matrix_lookup (data, dim, Int32Pair *, n, output) with pairs on the last row
    and column.  The pairs are arrays of the header's Int32Pair {first, second}.  (An n-term sum is held to
    (n + 2) u times the sum of magnitudes.)"""
    pair_t = np.dtype([("first", np.int32), ("second", np.int32)])
    X = rng.standard_normal((19, 120)).astype(real.np)
    x = real.mat(X, 4, 1)
    sizes = rng.multinomial(120, np.full(38, 1 / 38.0))
    ends = np.cumsum(sizes)
    pairs = np.zeros(40, pair_t)
    pairs["first"][:38], pairs["second"][:38] = ends - sizes, ends
    pairs[38], pairs[39] = (0, 120), (57, 57)
    assert pair_t.itemsize == 8 and (pairs["first"] == pairs["second"]).any()
    y = real.blank(19, 40, 3, 2)
    assert x.stride != y.stride
    call("sum_column_ranges", G, B, ptr(y), dim(y), ptr(x), dim(x), ptr(seam.torch.from_numpy(pairs.view(np.int32)).cuda()))
    done(seam, x, y)
    # an n-term sum: within (n + 2) u of the long-double value times the sum of magnitudes
    want = np.stack([X[:, b:e].astype(LD).sum(1) for b, e in pairs], 1)
    mag = np.stack([np.abs(X[:, b:e]).astype(LD).sum(1) for b, e in pairs], 1)
    excess = np.abs(y.host().astype(LD) - want) - (sizes_of(pairs) + 2) * real.u * mag
    assert excess.max() <= 0, "bound exceeded by %g" % float(excess.max())
    cases.exact(y.host()[:, 39], np.zeros(19, real.np))
    look = np.zeros(33, pair_t)
    look["first"], look["second"] = rng.integers(0, 19, 33), rng.integers(0, 120, 33)
    look[0], look[1], look[2] = (18, 119), (18, 0), (0, 119)
    out = real.blank(1, 33, 2, 1)
    call("matrix_lookup", G, B, ptr(x), dim(x), ptr(seam.torch.from_numpy(look.view(np.int32)).cuda()), 33, ptr(out))
    done(seam, x, out)
    cases.exact(out.host()[0], X[look["first"], look["second"]])
    cases.exact(x.host(), X)


# (name, transM, transN, N is M): the four forms of CuVectorBase::AddDiagMatMat (cu-vector.cc:533-580) and the two of
# AddDiagMat2 (:517-530), which calls it with N = M and the opposite transpose
DIAG_FORMS = [("NN", 0, 0, False), ("NT", 0, 1, False), ("TN", 1, 0, False), ("TT", 1, 1, False),
              ("AddDiagMat2 kNoTrans", 0, 1, True), ("AddDiagMat2 kTrans", 1, 0, True)]


@pytest.mark.parametrize("form", DIAG_FORMS, ids=[f[0].replace(" ", "_") for f in DIAG_FORMS])
def test_add_diag_mat_mat_forms(seam, call, real, rng, form):
    """v[i] = beta v[i] + alpha sum_j op(M)(i, j) op(N)(j, i) with the row and column strides cu-vector.cc:545-548
    derives: (Stride(), 1), swapped under kTrans.  M and N are different matrices with different strides; for float
    AddDiagMat2 kNoTrans takes the kh_add_diag_mat2 shortcut, everything else the general kernel.  beta = 0 over a
    NaN v, and v_dim = 0.  dim products and their sum, alpha times it, beta v, their sum: within (dim + 2) u of the
    long-double value times the sum of magnitudes."""
    _, tM, tN, same = form
    dim_v, dim_k = 19, 33
    Mh = rng.standard_normal((dim_k, dim_v) if tM else (dim_v, dim_k)).astype(real.np)
    Nh = Mh if same else rng.standard_normal((dim_v, dim_k) if tN else (dim_k, dim_v)).astype(real.np)
    m = real.mat(Mh, 3, 2)
    n = m if same else real.mat(Nh, 5, 1)
    assert same or m.stride != n.stride
    m_rs, m_cs = (1, m.stride) if tM else (m.stride, 1)
    n_rs, n_cs = (1, n.stride) if tN else (n.stride, 1)
    opM = (Mh.T if tM else Mh).astype(LD)
    opN = (Nh.T if tN else Nh).astype(LD)
    dot, mag = np.einsum("ij,ji->i", opM, opN), np.einsum("ij,ji->i", np.abs(opM), np.abs(opN))
    v0 = rng.standard_normal(dim_v).astype(real.np)
    for alpha, beta in ((0.5, 2.0), (0.75, 0.0)):
        v = dd.NanView(1, dim_v, dim_v + 2, 1, None if beta == 0.0 else v0[None, :], real.torch)
        call("add_diag_mat_mat", 1, 256, alpha, ptr(v), dim_v, ptr(m), dim_k, m_rs, m_cs, ptr(n), n_rs, n_cs, 1, beta)
        done(seam, v, m, n)
        got = v.host()[0]
        assert np.isfinite(got).all()
        vin = v0.astype(LD) if beta != 0.0 else np.zeros(dim_v, LD)
        excess = np.abs(got.astype(LD) - (alpha * dot + beta * vin)) - (dim_k + 2) * real.u * (alpha * mag + np.abs(beta * vin))
        assert excess.max() <= 0, "bound exceeded by %g" % float(excess.max())
    v = dd.NanView(1, dim_v, dim_v + 2, 1, v0[None, :], real.torch)
    call("add_diag_mat_mat", 1, 256, 0.5, ptr(v), 0, ptr(m), dim_k, m_rs, m_cs, ptr(n), n_rs, n_cs, 1, 2.0)   # v_dim = 0
    done(seam, v, m, n)
    cases.exact(v.host()[0], v0)
    cases.exact(m.host(), Mh)


@pytest.mark.parametrize("s", [0, 25, 2500])
def test_comp_obj_deriv(seam, call, real, rng, s):
    """CuMatrixBase::CompObjfAndDeriv (cu-matrix.cc:1198-1248): s MatrixElement<Real> {int32 row, int32 column, Real
    weight} on the device, the output z and the derivative z2 as views with different strides, t = 2 Reals that the
    kernel OVERWRITES.  s = 0 leaves {0, 0}; s = 25 is one partial wave without a repeated cell; s = 2500 draws from
    300 distinct cells, so every wave of the 1024-thread block is populated, the j += 1024 loop runs two or three
    times per thread and cells repeat about 8 times on average (atomicAdd).  z2 starts from a positive matrix.

    Bounds against long double.  z2: a cell hit `mult` times takes one division and mult additions of positive terms
    in any order: relative error at most (mult + 1) u; a cell not hit is unchanged.  t[1] = sum w is accumulated in
    double in both types, each term through at most 3 (thread) + 6 (wave butterfly) + 16 (the waves) = 25 additions:
    25 * 2^-53 * sum w, plus for float the final rounding u * sum w.  t[0] = sum w log z: each term is one log (the
    device's log / logf: at most 1 ulp = 2 u relative) and one product (u) in Real, then the same 25 double additions:
    double (2 + 1 + 25) * 2^-53 * sum |w log z|; float 3 * 2^-24 * (1 + 2^-22) * sum |w log z| + 25 * 2^-53 * sum |w log z|
    + the final rounding 2^-24 |t[0]|."""
    rows, cols = 19, 120
    P = (np.abs(rng.standard_normal((rows, cols))) + 0.05).astype(real.np)
    D0 = rng.uniform(0.5, 1.5, (rows, cols)).astype(real.np)
    cells = rng.permutation(rows * cols)[:300]
    pick = cells[:25] if s == 25 else cells[rng.integers(0, 300, s)]
    el = np.zeros(max(s, 1), dtype=[("row", np.int32), ("column", np.int32), ("weight", real.np)])
    assert el.dtype.itemsize == (16 if real.double else 12)
    el["row"][:s], el["column"][:s] = pick // cols, pick % cols
    el["weight"][:s] = rng.uniform(0.2, 1.5, s).astype(real.np)
    el = el[:s] if s else el
    r, c, w = el["row"][:s], el["column"][:s], el["weight"][:s].astype(LD)
    mult = np.zeros((rows, cols), np.int64)
    np.add.at(mult, (r, c), 1)
    if s == 25:
        assert mult.max() == 1
    if s == 2500:
        assert s > 2 * 1024 and mult.max() >= 12 and (mult > 0).sum() > 290
    d_el = seam.torch.from_numpy(np.ascontiguousarray(el).view(np.uint8).copy()).cuda()
    p, deriv, t = real.mat(P, 4, 1), real.mat(D0, 2, 2), real.blank(1, 2, 2, 1)
    assert p.stride != deriv.stride
    call("comp_obj_deriv", G, B, ptr(d_el), s, ptr(p), dim(p), ptr(deriv), dim(deriv), ptr(t))
    done(seam, p, deriv, t)
    cases.exact(p.host(), P)
    got_d, got_t = deriv.host(), t.host()[0].astype(LD)
    pr = P[r, c].astype(LD)
    want_d = D0.astype(LD)
    np.add.at(want_d, (r, c), w / pr)
    cases.exact(got_d[mult == 0], D0[mult == 0])
    excess = np.abs(got_d.astype(LD) / want_d - 1) - (mult + 1) * real.u
    assert excess[mult > 0].size == 0 or excess[mult > 0].max() <= 0, "deriv: bound exceeded by %g" % float(excess.max())
    terms = w * np.log(pr)
    objf, wsum, mag = terms.sum(), w.sum(), np.abs(terms).sum()
    if s == 0:
        assert got_t[0] == 0 and got_t[1] == 0
        return
    adds = 25 * U64
    if real.double:
        b0, b1 = (3 * U64 + adds) * mag, adds * wsum
    else:
        b0 = (3 * real.u * (1 + 2.0 ** -22) + adds) * mag + real.u * abs(objf)
        b1 = (adds + real.u) * wsum
    print("s = %d: |t[0] - truth| = %.3g (bound %.3g), |t[1] - truth| = %.3g (bound %.3g)" % (
        s, float(abs(got_t[0] - objf)), float(b0), float(abs(got_t[1] - wsum)), float(b1)))
    assert abs(got_t[0] - objf) <= b0 and abs(got_t[1] - wsum) <= b1


@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_as_add_mat_mat_issues_it(seam, call, real, oracle, rng, tA, tB):
    """CuMatrixBase::AddMatMat (cu-matrix.cc:947-982): cublas_gemm(transB, transA, m = C.cols, n = C.rows, k, alpha, B,
    B.Stride(), A, A.Stride(), beta, C, C.Stride()) on three sub-matrices, every ld > cols and all three different;
    beta = 0 over a NaN C.  Float: bit-exact against the oracle, as test_cublas_sgemm_as_cu_matrix_calls_it.  Both
    types: a K-term chain and the epilogue's three roundings, (K + 4) u S against long double (dense_dispatch.
    gemm_float64_bound restated)."""
    mm, nn, kk = 45, 70, 33
    A = rng.standard_normal((kk, mm) if tA else (mm, kk)).astype(real.np)
    Bm = rng.standard_normal((nn, kk) if tB else (kk, nn)).astype(real.np)
    C0 = rng.standard_normal((mm, nn)).astype(real.np)
    a, b = real.mat(A, 3, 1), real.mat(Bm, 5, 2)
    opA, opB = (A.T if tA else A).astype(LD), (Bm.T if tB else Bm).astype(LD)
    prod, mag = opA @ opB, np.abs(opA) @ np.abs(opB)
    for alpha, beta in ((0.5, 0.25), (0.75, 0.0)):
        c = dd.NanView(mm, nn, nn + 2, 1, None if beta == 0.0 else C0, real.torch)
        assert len({a.stride, b.stride, c.stride}) == 3 and a.stride > A.shape[1] and b.stride > Bm.shape[1]
        call("gemm", b"T" if tB else b"N", b"T" if tA else b"N", nn, mm, kk, alpha, ptr(b), b.stride, ptr(a), a.stride,
             beta, ptr(c), c.stride)
        done(seam, a, b, c)
        got = c.host()
        assert np.isfinite(got).all()
        c_in = C0 if beta != 0.0 else np.zeros_like(C0)
        if not real.double:
            cases.exact(got, oracle.add_mat_mat(alpha, A, tA, Bm, tB, beta, c_in))
        excess = (np.abs(got.astype(LD) - (alpha * prod + beta * c_in.astype(LD))) -
                  (kk + 4) * real.u * (alpha * mag + np.abs(beta * c_in)))
        assert excess.max() <= 0, "bound exceeded by %g" % float(excess.max())


def test_error_is_recorded_once_and_nothing_is_written(seam, call, real):
    """A bad argument (stride < cols): kh_cuda_seam_status() is non-zero once, then zero; the matrix is untouched."""
    m = real.mat(np.full((3, 5), 2.0), 2, 1)
    assert seam.lib.kh_cuda_seam_status() == 0
    call("apply_log", G, B, ptr(m), MatrixDim(3, 5, 4))
    assert seam.lib.kh_cuda_seam_status() != 0
    assert seam.lib.kh_cuda_seam_status() == 0
    seam.api.synchronize()
    m.assert_padding_untouched()
    cases.exact(m.host(), np.full((3, 5), 2.0, real.np))
