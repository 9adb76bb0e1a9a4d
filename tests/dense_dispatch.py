"""Helpers of test_gpu_dense_dispatch.py, test_gpu_double.py and test_gpu_cuda_seam.py.

1. The launch conditions of the dense forward-path kernels restated as pure functions of shapes, strides and base
   pointers (each cites the source line it mirrors), so a test can assert that its operands land in the branch it is
   about BEFORE it calls the kernel: a case that drifts out of its branch (the allocator's alignment, a changed
   threshold) then fails loudly instead of passing on another path.
2. NanView: an operand as a view into a NaN-filled buffer, with a chosen row stride (padding) and base offset (a
   column offset of 1-3 elements, what a CuSubMatrix caller passes); after the call the padding must still be NaN.
   float32 unless a dtype is given."""
import numpy as np
import torch

NAN = float("nan")


NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}


class NanView:
    """rows x cols device view (float32, or `dtype`) with row stride `stride` starting `offset` elements into a
    NaN-filled buffer."""

    def __init__(self, rows, cols, stride=None, offset=0, host=None, dtype=torch.float32):
        stride = cols if stride is None else stride
        assert stride >= cols and offset >= 0
        self.shape, self.stride, self.offset, self.dtype = (rows, cols), stride, offset, dtype
        self.buf = torch.full((offset + rows * stride,), NAN, dtype=dtype, device="cuda")
        self.t = self._view(self.buf)
        if host is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(host, NP_DTYPE[dtype])))
        assert self.t.data_ptr() == self.buf.data_ptr() + self.buf.element_size() * offset
        assert rows <= 1 or self.t.stride(0) == stride

    def _view(self, buf):
        return buf.as_strided(self.shape, (self.stride, 1), self.offset)

    def host(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().copy()

    def assert_padding_untouched(self):
        """Every float of the buffer outside the view is still NaN: nothing was stored outside the view."""
        torch.cuda.synchronize()
        chk = self.buf.clone()
        self._view(chk).fill_(NAN)
        bad = int((~torch.isnan(chk)).sum())
        assert bad == 0, "%d floats outside the %dx%d view (stride %d, offset %d) were written" % (
            (bad,) + self.shape + (self.stride, self.offset))


def mat(host, pad=0, offset=0, dtype=torch.float32):
    """Host matrix -> NanView with `pad` elements of row padding and a base offset of `offset` elements."""
    host = np.ascontiguousarray(host, NP_DTYPE[dtype])
    return NanView(host.shape[0], host.shape[1], host.shape[1] + pad, offset, host, dtype)


def vec(host, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(host, NP_DTYPE[dtype])).cuda()


def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stride0(t):
    # api._dim: the stride handed to the library (a one-row tensor reports max(stride, cols))
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


# ---------------------------------------------------------------- kh_gemm.hip
BM = BN = 128          # kh_gemm.hip:35
PBM, PBN = 128, 160    # kh_gemm.hip:268


def gemm_launch(A, transA, B, transB):
    """What LaunchGemm decides for kh_add_mat_mat / kh_affine (kh_affine: transA = 0, transB = 1)."""
    m, k = (A.shape[1], A.shape[0]) if transA else A.shape
    n = B.shape[0] if transB else B.shape[1]
    a_si, a_sk = (1, _stride0(A)) if transA else (_stride0(A), 1)      # kh_gemm.hip:445-446
    b_sj, b_sk = (_stride0(B), 1) if transB else (1, _stride0(B))      # kh_gemm.hip:447-448
    d = dict(m=m, n=n, k=k)
    d["lane_offsets_ok"] = 0 <= a_si < (1 << 22) and 0 <= b_sj < (1 << 22)          # kh_gemm.hip:404
    d["va"] = a_sk == 1 and a_si % 4 == 0 and A.data_ptr() % 16 == 0                 # kh_gemm.hip:405-406
    d["vb"] = b_sk == 1 and b_sj % 4 == 0 and B.data_ptr() % 16 == 0                 # kh_gemm.hip:407-408
    tiles_m, tiles_n = -(-m // BM), -(-n // BN)                                      # kh_gemm.hip:401-402
    d["tiles"] = tiles_m * tiles_n
    full = (m // BM) * (n // BN)          # tiles with rowsA >= BM && rowsB >= BN
    d["full_tiles"] = full
    d["interior_tiles"] = full if d["va"] and d["vb"] and d["lane_offsets_ok"] else 0  # kh_gemm.hip:126
    d["setprio_arms"] = min(4, -(-d["tiles"] // 256))    # (blockIdx.x >> 8) & 3 takes this many values, kh_gemm.hip:93
    d["xcd_remap_uneven"] = d["tiles"] % 8 != 0          # rem != 0: both arms of XcdRemap, kh_gemm.hip:56-59
    return d


def affine_pnorm_launch(A, W):
    """What kh_affine_pnorm decides."""
    m, n = A.shape[0], W.shape[0]
    a_si, b_sj = _stride0(A), _stride0(W)
    d = dict(tiles=-(-m // PBM) * -(-n // PBN))                                      # kh_gemm.hip:507-508
    d["lane_offsets_ok"] = a_si < (1 << 22) and b_sj < (1 << 22)                    # kh_gemm.hip:509
    d["vec"] = (a_si % 4 == 0 and b_sj % 4 == 0 and A.data_ptr() % 16 == 0 and      # kh_gemm.hip:513-514
                W.data_ptr() % 16 == 0)
    d["interior_tiles"] = (m // PBM) * (n // PBN) if d["vec"] and d["lane_offsets_ok"] else 0  # kh_gemm.hip:299
    return d


# ---------------------------------------------------------------- output layer
SOFTMAX_LDS_COLS = 12288   # kSoftmaxLdsFloats, kh_elementwise.hip:38
K_PRE = 12                 # kPre, kh_elementwise.hip:106


def output_layer_launch(n_mix, n_pdf, x_ptr_aligned=True):
    """Softmax -> sum-group as the last two components of a network (NnetComputeImpl).  The logits are the library's
    own buffer: its row stride is Pad4(n_mix) (kh_nnet.hip:488) and its base comes from the device pool, so the
    pointer term of the float4 condition is not visible from here; n_mix % 4 != 0 alone forces the scalar pass."""
    d = dict(fused=n_mix <= SOFTMAX_LDS_COLS)                                        # kh_nnet.hip:553
    d["block"] = 512 if n_mix > 4096 else 256                                        # kh_elementwise.hip:418
    d["pre"] = n_pdf <= K_PRE * d["block"]                                           # kh_elementwise.hip:107
    x_stride = (n_mix + 3) // 4 * 4
    d["float4_load"] = n_mix % 4 == 0 and x_stride % 4 == 0 and x_ptr_aligned        # kh_elementwise.hip:124
    return d


def softmax_kernel(cols):
    """The kernel kh_softmax_per_row / kh_log_softmax_per_row launch (kh_elementwise.hip:436-446, :458-468) and, for the
    block kernel, whether the row is held in LDS (:52)."""
    if cols <= 1024:
        return "SoftmaxWaveKernel"
    return "SoftmaxKernel<%d>%s" % (512 if cols > 4096 else 256, "" if cols <= SOFTMAX_LDS_COLS else " uncached")


def max_group(sizes):
    return int(np.max(sizes))   # > 4: the tail loop of emit(), kh_elementwise.hip:177-181


# ---------------------------------------------------------------- kh_group_pnorm
PNORM_LDS_FLOATS = 4096    # kPnormLdsFloats, kh_elementwise.hip:260


def pnorm_kernel(power, in_cols):
    """The kernel kh_group_pnorm launches (kh_elementwise.hip:512-523)."""
    if power == 2.0 and 512 <= in_cols <= PNORM_LDS_FLOATS:
        return "GroupPnorm2RowKernel"
    return "GroupPnormKernel<%d>" % (0 if power == 2.0 else 1 if power == 1.0 else 2)


# ---------------------------------------------------------------- grid-stride loops
def map2d_grid(rows, cols):
    """LaunchMap2D's grid (kh_elementwise.hip:244-252) -> (gx, gy, columns per pass)."""
    bx = 256 if cols >= 256 else 64
    gx = min(-(-cols // bx), 64)
    gy = rows
    max_blocks = num_cus() * 16
    if gx * gy > max_blocks:
        gy = max(max_blocks // gx, 1)
    gy = min(gy, 65535)
    return gx, gy, gx * bx


def map2d_strides(rows, cols):
    """(rows need the row grid-stride loop, columns need the column grid-stride loop) of Map2D, :236-237."""
    gx, gy, cpp = map2d_grid(rows, cols)
    return rows > gy, cols > cpp


def rowcol_strides(rows, cols):
    """The same for RowColGrid (kh_elementwise.hip:395-402) with 256-thread blocks."""
    gx = min(-(-cols // 256), 32)
    gy = min(rows, max(num_cus() * 16 // gx, 1))
    return rows > gy, cols > gx * 256


def wave_row_stride(rows):
    """NormalizeKernel / AddDiagMat2Kernel: one wave per row, 4 per block, at most NumCUs()*8 blocks
    (kh_elementwise.hip:535-536, :549-550): more rows than wave slots take the grid-stride loop (:335-336, :357-358)."""
    return rows > min(-(-rows // 4), num_cus() * 8) * 4


# ---------------------------------------------------------------- kh_double.hip
# LaunchMap (kh_double.hip:149-160) is LaunchMap2D (kh_elementwise.hip:244-252) line for line: 256 threads from 256
# columns on and 64 below, gx = min(DivUp(cols, bx), 64), gy = rows cut to NumCUs()*16 / gx blocks (at least 1) and to
# 65535; Map2DD (:143-146) walks the same two grid-stride loops as Map2D.  So the float predicates are the double ones.
map_d_grid = map2d_grid
map_d_strides = map2d_strides


def add_diag_mat2_d_row_loop(rows):
    """AddDiagMat2DKernel: one wave per row, 4 per block, at most NumCUs()*8 blocks (kh_double.hip:301): more rows than
    wave slots take the grid-stride loop (:201)."""
    return rows > min(-(-rows // 4), num_cus() * 8) * 4


def lookup_d_loop(n):
    """LookupDKernel: one pair per thread, 256 per block, at most NumCUs()*8 blocks (kh_double.hip:353): more pairs than
    threads take the grid-stride loop (:213)."""
    return n > min(-(-n // 256), num_cus() * 8) * 256


# ---------------------------------------------------------------- references
U = 2.0 ** -24   # unit roundoff of float32


def gemm_float64_bound(alpha, A, transA, B, transB, beta, C0):
    """(R, bound): R = alpha op(A) op(B) + beta C0 in float64 and the elementwise error bound of a K-term fma chain
    plus the three roundings of the epilogue (alpha * acc, beta * c, their sum): (K + 4) u S with
    S = |alpha| |op(A)| |op(B)| + |beta| |C0|."""
    a = np.asarray(A, np.float64)
    b = np.asarray(B, np.float64)
    a = a.T if transA else a          # [m, k]
    b = b.T if transB else b          # [k, n]
    K = a.shape[1]
    c0 = np.asarray(C0, np.float64)
    c0 = np.where(np.isnan(c0), 0.0, c0) if beta == 0 else c0
    R = alpha * (a @ b) + beta * c0
    S = abs(alpha) * (np.abs(a) @ np.abs(b)) + abs(beta) * np.abs(c0)
    return R, (K + 4) * U * S
