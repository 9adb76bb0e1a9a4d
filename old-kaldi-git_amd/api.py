"""Python host-side mirror of the reference's operator interface for the hot path.

Same names / argument meaning / error behaviour as the reference classes
(`CuMatrixBase` methods of cudamatrix/cu-matrix.h, `cu::Splice`, `DiagGmm`,
`nnet2::Nnet` + `NnetComputation` + `DecodableAmNnet`, `LatticeFasterDecoder`,
`LatticeForwardBackward`), implemented by calling the C-ABI of libkaldi_hip.so.
torch is used only as the owner of device memory (tensors -> data_ptr()) and of
the HIP stream; no computation is done by torch and there is no fallback: every
function raises KhError (the KALDI_ERR equivalent) if the library call fails.
"""
import contextlib
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

from . import capi
from .capi import KhMatrixDim, KhComponentDesc, KhDecoderConfig, KhDecodeStats, check, KhError

kTrans, kNoTrans = 1, 0

TYPE_BY_NAME = {
    "splice": 1, "fixed_affine": 2, "affine": 3, "pnorm": 4, "normalize": 5,
    "softmax": 6, "sum_group": 7, "fixed_scale": 8, "fixed_bias": 9,
}


def lib():
    return capi.load()


def use_torch_stream():
    """Enqueue library work on torch's current HIP stream (ordering with tensor
    creation / copies done by torch)."""
    check(lib().kh_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def synchronize():
    """Wait for the library's stream (CU_SAFE_CALL's cudaThreadSynchronize, cu-common.h:37-44)."""
    check(lib().kh_synchronize())


def pool_release():
    """Return the blocks cached by the library's device-memory pool to the driver (kh_pool_release)."""
    check(lib().kh_pool_release())


def select_gpu(ordinal):
    """CuDevice::SelectGpuId with explicit ordinal (cu-device.cc:93-192)."""
    check(lib().kh_select_gpu(int(ordinal)))
    torch.cuda.set_device(int(ordinal))
    use_torch_stream()


def _fn(name, t, *others):
    """The entry point for the tensors' element type: kh_<name> (float) or its <double> twin kh_<name>_d.  Every
    floating-point operand of the call must have that one type (a float operand handed to the double kernel - or the
    other way round - would be reinterpreted, not converted)."""
    for o in others:
        assert not o.dtype.is_floating_point or o.dtype == t.dtype, "operands of different element types: %s and %s" % (t.dtype, o.dtype)
    if t.dtype == torch.float64:
        return getattr(lib(), name + "_d")
    assert t.dtype == torch.float32
    return getattr(lib(), name)


def _dim(t, dtype=torch.float32):
    """MatrixDim of a 2-D device tensor of element type `dtype` - float32 unless the caller dispatches on the type (_fn):
    the entry points without a <double> twin (affine, the network, the decoder, the GMM, iVectors, lattices) take float only."""
    assert t.dim() == 2 and t.dtype == dtype and t.is_cuda, "a 2-D %s device tensor is expected, got %s" % (dtype, t.dtype)
    assert t.stride(1) == 1 or t.shape[1] <= 1
    return KhMatrixDim(t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _p(t):
    return C.c_void_p(t.data_ptr())


def _dev_i32(a, device):
    if isinstance(a, torch.Tensor):
        assert a.dtype == torch.int32 and a.is_cuda
        return a
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=device)


# ---------------------------------------------------------------- CuMatrix ops
def add_mat_mat(Cm, alpha, A, transA, B, transB, beta):
    """CuMatrixBase::AddMatMat (cu-matrix.cc:947-982): C = alpha op(A) op(B) + beta C."""
    check(_fn("kh_add_mat_mat", Cm, A, B)(alpha, _p(A), _dim(A, Cm.dtype), int(transA), _p(B), _dim(B, Cm.dtype), int(transB), beta, _p(Cm), _dim(Cm, Cm.dtype)))
    return Cm


def affine(out, A, W, bias):
    check(lib().kh_affine(_p(A), _dim(A), _p(W), _dim(W), _p(bias), _p(out), _dim(out)))


def affine_pnorm(out, A, W, bias):
    """AffineComponent + PnormComponent (p = 2) in one kernel: out[r][c] = 2-norm of group c of row r of A W^T + bias
    (nnet-component.cc:1219-1224, :386-391); group size = W.shape[0] // out.shape[1]."""
    check(lib().kh_affine_pnorm(_p(A), _dim(A), _p(W), _dim(W), _p(bias), _p(out), _dim(out), W.shape[0] // out.shape[1]))
    return out


def apply_softmax_per_row(dst, src):
    """CuMatrixBase::ApplySoftMaxPerRow (cu-matrix.cc:1251-1271)."""
    assert dst.shape == src.shape  # KALDI_ASSERT(SameDim(*this, src))
    check(_fn("kh_softmax_per_row", dst, src)(_p(dst), _p(src), _dim(dst, dst.dtype), _dim(src, dst.dtype).stride))
    return dst


def apply_log_softmax_per_row(dst, src):
    assert dst.shape == src.shape
    check(_fn("kh_log_softmax_per_row", dst, src)(_p(dst), _p(src), _dim(dst, dst.dtype), _dim(src, dst.dtype).stride))
    return dst


def copy_rows(dst, src, indices):
    """CuMatrixBase::CopyRows (cu-matrix.cc:1965-1990)."""
    idx = _dev_i32(indices, dst.device)
    if dst.shape[1] != src.shape[1] or dst.shape[0] != idx.numel():
        raise KhError("CopyRows: dimension mismatch")
    check(_fn("kh_copy_rows", dst, src, idx)(_p(dst), _dim(dst, dst.dtype), _p(src), _dim(src, dst.dtype).stride, _p(idx)))
    return dst


def splice(src, frame_offsets, tgt):
    """cu::Splice (cudamatrix/cu-math.cc:130-165)."""
    off = _dev_i32(frame_offsets, src.device)
    check(_fn("kh_splice", tgt, src, off)(_p(tgt), _dim(tgt, tgt.dtype), _p(src), _dim(src, tgt.dtype), _p(off), off.numel()))
    return tgt


def group_pnorm(dst, src, power):
    """CuMatrixBase::GroupPnorm (cu-matrix.cc:1147-1164)."""
    if src.shape[1] % dst.shape[1] != 0 or src.shape[0] != dst.shape[0]:
        raise KhError("GroupPnorm: dimension mismatch")
    check(_fn("kh_group_pnorm", dst, src)(_p(dst), _p(src), _dim(dst, dst.dtype), _dim(src, dst.dtype).stride, src.shape[1] // dst.shape[1], power))
    return dst


def normalize(dst, src):
    """NormalizeComponent::Propagate (nnet2/nnet-component.cc:576-588)."""
    assert dst.shape == src.shape
    check(lib().kh_normalize(_p(dst), _p(src), _dim(dst), _dim(src).stride))
    return dst


def add_diag_mat2(v, alpha, M, beta):
    """CuVectorBase::AddDiagMat2 kNoTrans (cu-vector.cc:517-580)."""
    assert v.numel() == M.shape[0]
    check(_fn("kh_add_diag_mat2", M, v)(alpha, _p(M), _dim(M, M.dtype), beta, _p(v)))
    return v


def mul_rows_vec(M, s):
    assert s.numel() == M.shape[0]
    check(_fn("kh_mul_rows_vec", M, s)(_p(M), _dim(M, M.dtype), _p(s)))
    return M


def mul_cols_vec(M, s):
    assert s.numel() == M.shape[1]
    check(_fn("kh_mul_cols_vec", M, s)(_p(M), _dim(M, M.dtype), _p(s)))
    return M


def copy_rows_from_vec(M, v):
    assert v.numel() == M.shape[1]
    check(_fn("kh_copy_rows_from_vec", M, v)(_p(M), _dim(M, M.dtype), _p(v)))
    return M


def add_vec_to_rows(M, alpha, v, beta=1.0):
    assert v.numel() == M.shape[1]
    check(_fn("kh_add_vec_to_rows", M, v)(alpha, _p(v), beta, _p(M), _dim(M, M.dtype)))
    return M


def apply_floor(M, f):
    check(_fn("kh_apply_floor", M)(_p(M), _dim(M, M.dtype), f))
    return M


def apply_log(M):
    check(_fn("kh_apply_log", M)(_p(M), _dim(M, M.dtype)))
    return M


def apply_exp(M):
    check(_fn("kh_apply_exp", M)(_p(M), _dim(M, M.dtype)))
    return M


def apply_pow(M, p):
    check(_fn("kh_apply_pow", M)(_p(M), _dim(M, M.dtype), p))
    return M


def scale(M, a):
    check(_fn("kh_scale", M)(_p(M), _dim(M, M.dtype), a))
    return M


def sum_column_ranges(dst, src, ranges):
    """CuMatrixBase::SumColumnRanges (cu-matrix.cc:1994-2028)."""
    r = _dev_i32(ranges, dst.device)
    assert r.numel() == 2 * dst.shape[1]
    check(_fn("kh_sum_column_ranges", dst, src, r)(_p(dst), _dim(dst, dst.dtype), _p(src), _dim(src, dst.dtype), _p(r)))
    return dst


def lookup(M, pairs):
    """CuMatrixBase::Lookup (cu-matrix.cc:2327)."""
    pr = _dev_i32(pairs, M.device)
    n = pr.numel() // 2
    out = torch.empty(n, dtype=M.dtype, device=M.device)
    check(_fn("kh_matrix_lookup", M, pr, out)(_p(M), _dim(M, M.dtype), _p(pr), n, _p(out)))
    return out


# ---------------------------------------------------------------- nnet2
class Nnet:
    """nnet2::Nnet (forward only) + NnetComputation + DecodableAmNnet epilogue."""

    def __init__(self, components, priors=None):
        self._h = C.c_void_p(lib().kh_nnet_create())
        self._keep = []
        for comp in components:
            d = KhComponentDesc()
            d.type = TYPE_BY_NAME[comp["type"]]
            d.input_dim, d.output_dim = int(comp["input_dim"]), int(comp["output_dim"])
            keep = []
            if "linear" in comp:
                w = np.ascontiguousarray(comp["linear"], np.float32)
                keep.append(w)
                d.linear = w.ctypes.data_as(capi.c_float_p)
            if "bias" in comp:
                b = np.ascontiguousarray(comp["bias"], np.float32)
                keep.append(b)
                d.bias = b.ctypes.data_as(capi.c_float_p)
            if "context" in comp:
                ctx = np.ascontiguousarray(comp["context"], np.int32)
                keep.append(ctx)
                d.context = ctx.ctypes.data_as(capi.c_int32_p)
                d.n_context = len(ctx)
                d.const_dim = int(comp.get("const_dim", 0))
            d.p = float(comp.get("p", 2.0))
            if "sizes" in comp:
                sz = np.ascontiguousarray(comp["sizes"], np.int32)
                keep.append(sz)
                d.sizes = sz.ctypes.data_as(capi.c_int32_p)
                d.n_sizes = len(sz)
            check(lib().kh_nnet_add_component(self._h, C.byref(d)))
        if priors is not None:
            pr = np.ascontiguousarray(priors, np.float32)
            check(lib().kh_nnet_set_priors(self._h, pr.ctypes.data_as(capi.c_float_p), len(pr)))

    def __del__(self):
        try:
            if self._h:
                lib().kh_nnet_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def input_dim(self):
        return lib().kh_nnet_input_dim(self._h)

    def output_dim(self):
        return lib().kh_nnet_output_dim(self._h)

    def left_context(self):
        return lib().kh_nnet_left_context(self._h)

    def right_context(self):
        return lib().kh_nnet_right_context(self._h)

    def compute(self, feats, utt_row_offsets=None, pad_input=True, epilogue=False, prob_scale=1.0, out=None, wait=True):
        """NnetComputation (nnet-compute.cc:159-166) for a batch stacked by rows;
        epilogue=True adds DecodableAmNnet's floor/log/-logprior/scale.
        wait=False: kh_nnet_compute_async - the call returns when the work is queued on the library's stream."""
        T = feats.shape[0]
        if utt_row_offsets is None:
            utt_row_offsets = [0, T]
        off = np.ascontiguousarray(utt_row_offsets, np.int32)
        n_utts = len(off) - 1
        L, R = self.left_context(), self.right_context()
        rows = int(off[-1] - off[0]) if pad_input else int(off[-1] - off[0]) - n_utts * (L + R)
        if rows <= 0:
            raise KhError("Nnet.compute: no output rows")
        if out is None:
            od = self.output_dim()
            stride = (od + 3) // 4 * 4
            out = torch.empty((rows, stride), dtype=torch.float32, device=feats.device)[:, :od]
        out_off = np.zeros(n_utts + 1, np.int32)
        check((lib().kh_nnet_compute if wait else lib().kh_nnet_compute_async)(self._h, _p(feats), _dim(feats).stride,
                                    off.ctypes.data_as(capi.c_int32_p), n_utts, int(pad_input),
                                    int(epilogue), float(prob_scale), _p(out), _dim(out).stride,
                                    out_off.ctypes.data_as(capi.c_int32_p)))
        return out, out_off


class DecodableNnet2Online:
    """nnet2/online-nnet2-decodable.{h,cc} for num_streams concurrent utterances: the
    feature rows of a stream arrive in chunks (the OnlineFeatureInterface side:
    accept_features / input_finished), NumFramesReady() follows :75-89, and compute()
    is ComputeForFrame (:91-143) for a list of streams at once — one gather of the
    context-padded input rows (first / last frame duplicated past the edges when
    pad_input), one NnetComputation(pad_input=false) over all of them, the
    floor / log / -log prior / acoustic scale epilogue."""

    def __init__(self, nnet, num_streams, max_frames, acoustic_scale=0.1, pad_input=True, max_nnet_batch_size=256,
                 device="cuda"):
        assert max_nnet_batch_size > 0  # :40
        self.nnet, self.scale, self.pad_input, self.max_batch = nnet, float(acoustic_scale), bool(pad_input), int(max_nnet_batch_size)
        self.num_streams, self.max_frames = int(num_streams), int(max_frames)
        self.L, self.R = nnet.left_context(), nnet.right_context()
        dim = nnet.input_dim()
        stride = (dim + 3) // 4 * 4
        self._feats = torch.empty((self.num_streams * self.max_frames, stride), dtype=torch.float32, device=device)[:, :dim]
        self._n = [0] * self.num_streams
        self._finished = [False] * self.num_streams

    def reset(self, streams):
        for s in streams:
            self._n[s], self._finished[s] = 0, False

    def accept_features(self, stream, feats, input_finished=False):
        """Append rows (host array or device tensor) to the stream's features."""
        assert not self._finished[stream], "input already finished"
        x = feats if torch.is_tensor(feats) else torch.from_numpy(np.ascontiguousarray(feats, np.float32))
        k = x.shape[0]
        if self._n[stream] + k > self.max_frames:
            raise KhError("DecodableNnet2Online: more than max_frames=%d feature frames" % self.max_frames)
        if k:
            b = stream * self.max_frames + self._n[stream]
            self._feats[b:b + k].copy_(x)
        self._n[stream] += k
        self._finished[stream] = bool(input_finished)

    def accept_features_many(self, streams, src, src_rows, counts, finished):
        """accept_features for many streams with ONE device copy: streams[i] takes rows [src_rows[i], src_rows[i] + counts[i])
        of the device matrix `src` (what a batched feature front end hands over per chunk); finished[i]: InputFinished()."""
        src_idx, dst_idx = [], []
        for s, r, k, fin in zip(streams, src_rows, counts, finished):
            assert not self._finished[s], "input already finished"
            if self._n[s] + k > self.max_frames:
                raise KhError("DecodableNnet2Online: more than max_frames=%d feature frames" % self.max_frames)
            if k:
                src_idx.append(np.arange(r, r + k))
                dst_idx.append(s * self.max_frames + self._n[s] + np.arange(k))
            self._n[s] += int(k)
            self._finished[s] = bool(fin)
        if src_idx:
            si = torch.from_numpy(np.concatenate(src_idx)).to(self._feats.device)
            di = torch.from_numpy(np.concatenate(dst_idx)).to(self._feats.device)
            self._feats.index_copy_(0, di, src.index_select(0, si))

    def num_frames_ready(self, stream):
        """NumFramesReady() :75-89."""
        ready = self._n[stream]
        if ready == 0:
            return 0
        if self.pad_input:
            return ready if self._finished[stream] else max(0, ready - self.R)
        return max(0, ready - self.R - self.L)

    def is_last_frame(self, stream, frame):
        """IsLastFrame() :67-73."""
        last = self._n[stream] - 1 if self._finished[stream] else None
        if last is None:
            return False
        return frame == last if self.pad_input else frame + self.L + self.R == last

    def compute(self, streams, frames):
        """Scaled log-likelihoods of frames [frames[i], frames[i] + n_i) of streams[i],
        n_i = min(NumFramesReady - frames[i], max_nnet_batch_size) (ComputeForFrame).
        Returns one device matrix per stream (0 rows if nothing is ready)."""
        idx, off, n_out = [], [0], []
        for s, f in zip(streams, frames):
            ready = self._n[s]
            n = max(0, min(self.num_frames_ready(s) - f, self.max_batch))
            n_out.append(n)
            if n == 0:
                continue
            begin = f - self.L if self.pad_input else f          # :103-107
            t = np.arange(begin, begin + n + self.L + self.R)
            t = np.clip(t, 0, ready - 1)                            # :118-124 (only ever clips when pad_input)
            idx.append(s * self.max_frames + t)
            off.append(off[-1] + len(t))
        od = self.nnet.output_dim()
        if not idx:
            return [torch.empty((0, od), dtype=torch.float32, device=self._feats.device) for _ in streams]
        idx = np.concatenate(idx).astype(np.int32)
        stride = self._feats.stride(0)
        x = torch.empty((len(idx), stride), dtype=torch.float32, device=self._feats.device)[:, :self._feats.shape[1]]
        copy_rows(x, self._feats, idx)
        out, out_off = self.nnet.compute(x, off, pad_input=False, epilogue=True, prob_scale=self.scale)
        res, k = [], 0
        for n in n_out:
            if n == 0:
                res.append(out[0:0])
            else:
                res.append(out[int(out_off[k]):int(out_off[k]) + n])
                k += 1
        return res


class OnlineNnet2Pipeline:
    """The serving loop of online2-wav-nnet2-latgen-faster (:213-262) for num_streams concurrent utterances with ONE library
    call per step (kh_online_nnet2_*): step() hands every live stream its chunk of feature rows, DecodableNnet2Online's
    ComputeForFrame runs for all advancing streams in one forward pass, AdvanceDecoding consumes the frames.  `decoder` is a
    LatticeFasterOnlineDecoder (results are read from it: get_best_path, get_raw_lattice, finalize_decoding)."""

    def __init__(self, nnet, decoder, max_frames, acoustic_scale=0.1, pad_input=True, max_nnet_batch_size=256):
        self.nnet, self.decoder = nnet, decoder
        h = lib().kh_online_nnet2_create(nnet._h, decoder._h, decoder.num_streams, int(max_frames), float(acoustic_scale),
                                         int(bool(pad_input)), int(max_nnet_batch_size))
        if not h:
            raise KhError(lib().kh_last_error().decode())
        self._h = C.c_void_p(h)
        fst = decoder.fst
        self._t2p = _p(fst.tid2pdf) if fst.tid2pdf is not None else None
        fst.check_pdf_map(nnet.output_dim())
        # the decoder's arc records for this (map, columns) pair once, not at every chunk
        check(lib().kh_online_decoder_set_pdf_map(decoder._h, self._t2p, (nnet.output_dim() + 3) // 4 * 4))

    def __del__(self):
        try:
            if self._h:
                lib().kh_online_nnet2_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def reset(self, streams):
        st = np.ascontiguousarray(streams, np.int32)
        check(lib().kh_online_nnet2_reset(self._h, st.ctypes.data_as(capi.c_int32_p), len(st)))

    def step(self, streams, src, src_rows, counts, finished):
        """streams[i] receives rows [src_rows[i], src_rows[i] + counts[i]) of the device matrix src; finished[i]:
        InputFinished().  Returns NumFramesDecoded() of the listed streams after the step."""
        st = np.ascontiguousarray(streams, np.int32)
        sr = np.ascontiguousarray(src_rows, np.int32)
        ct = np.ascontiguousarray(counts, np.int32)
        fi = np.ascontiguousarray(finished, np.int32)
        out = np.empty(len(st), np.int32)
        ip = capi.c_int32_p
        check(lib().kh_online_nnet2_step(self._h, st.ctypes.data_as(ip), len(st), _p(src), _dim(src).stride, sr.ctypes.data_as(ip),
                                         ct.ctypes.data_as(ip), fi.ctypes.data_as(ip), self._t2p, out.ctypes.data_as(ip)))
        return out

    # ---- serving through the decoder's persistent kernel (kh_online_nnet2_serve_*): step() then returns once the chunk's
    # scores are published, the decoder follows at its own pace (a stream that prunes does not hold up the others)
    def serve_start(self):
        check(lib().kh_online_nnet2_serve_start(self._h, self._t2p))

    def serve_stop(self):
        check(lib().kh_online_nnet2_serve_stop(self._h))

    def serve_finalize(self, streams):
        """FinalizeDecoding of the streams once everything submitted to them is decoded (asynchronous)."""
        st = np.ascontiguousarray(streams, np.int32)
        check(lib().kh_online_nnet2_serve_finalize(self._h, st.ctypes.data_as(capi.c_int32_p), len(st)))

    def serve_poll(self, streams):
        """(NumFramesDecoded() so far, request still in flight) of the streams."""
        st = np.ascontiguousarray(streams, np.int32)
        dec, fl = np.empty(len(st), np.int32), np.empty(len(st), np.int32)
        ip = capi.c_int32_p
        check(lib().kh_online_nnet2_serve_poll(self._h, st.ctypes.data_as(ip), len(st), dec.ctypes.data_as(ip), fl.ctypes.data_as(ip)))
        return dec, fl.astype(bool)

    def serve_wait(self, streams, timeout_ms=0):
        st = np.ascontiguousarray(streams, np.int32)
        check(lib().kh_online_nnet2_serve_wait(self._h, st.ctypes.data_as(capi.c_int32_p), len(st), int(timeout_ms)))


# ---------------------------------------------------------------- feature front-end
class Mfcc:
    """feat/feature-mfcc.h Mfcc with MfccOptions: the constructor builds the reference's tables
    (window function, MelBanks, DCT rows, lifter) on the host, compute() runs the frames on the
    GPU.  Defaults here are the recipes' (--use-energy=false, no dither); the reference's
    struct defaults are use_energy = true, dither = 1.0 (feature-mfcc.h:54, feature-functions.h:91).
    dither > 0 draws from a counter-based generator seeded with dither_seed."""

    def __init__(self, samp_freq=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, preemph_coeff=0.97,
                 remove_dc_offset=True, window_type="povey", num_bins=23, low_freq=20.0, high_freq=0.0, num_ceps=13,
                 cepstral_lifter=22.0, snip_edges=True, use_energy=False, raw_energy=True, energy_floor=0.0,
                 htk_compat=False, dither=0.0, dither_seed=0):
        f32 = np.float32
        self.opts = capi.KhMfccOptions(int(snip_edges), int(use_energy), int(raw_energy), int(htk_compat),
                                       float(energy_floor), float(dither), int(dither_seed))
        self.samp_freq = float(samp_freq)
        self.frame_shift = int(f32(samp_freq) * f32(0.001) * f32(frame_shift_ms))      # WindowShift() feature-functions.h:119
        self.frame_length = int(f32(samp_freq) * f32(0.001) * f32(frame_length_ms))    # WindowSize()
        self.padded = 1 << int(np.ceil(np.log2(self.frame_length)))                    # PaddedWindowSize()
        self.preemph, self.remove_dc = float(preemph_coeff), bool(remove_dc_offset)
        self.num_bins, self.num_ceps = int(num_bins), int(num_ceps)
        n = self.frame_length
        i = np.arange(n, dtype=np.float32).astype(np.float64)
        a = 2.0 * np.pi * i / (n - 1)
        if window_type == "hanning":                                                    # FeatureWindowFunction :74-92
            w = 0.5 - 0.5 * np.cos(a)
        elif window_type == "hamming":
            w = 0.54 - 0.46 * np.cos(a)
        elif window_type == "povey":
            w = np.power(0.5 - 0.5 * np.cos(a), 0.85)
        elif window_type == "rectangular":
            w = np.ones(n)
        else:
            raise KhError("Invalid window type " + window_type)
        self.window = w.astype(np.float32)
        # MelBanks (vtln_warp 1.0) mel-computations.cc:33-152, float arithmetic as there
        mel = lambda fr: f32(1127.0) * np.log(f32(1.0) + np.asarray(fr, np.float32) / f32(700.0), dtype=np.float32)
        nyquist = f32(0.5) * f32(samp_freq)
        hf = f32(high_freq) if high_freq > 0.0 else nyquist + f32(high_freq)
        lf = f32(low_freq)
        if lf < 0.0 or lf >= nyquist or hf <= 0.0 or hf > nyquist or hf <= lf:
            raise KhError("Bad values in options: low-freq %g and high-freq %g vs. nyquist %g" % (lf, hf, nyquist))
        num_fft_bins = self.padded // 2
        fft_bin_width = f32(samp_freq) / f32(self.padded)
        mel_low, mel_high = mel(lf), mel(hf)
        delta = (mel_high - mel_low) / f32(num_bins + 1)
        mels = mel(fft_bin_width * np.arange(num_fft_bins, dtype=np.float32))
        first, off, weights = [], [0], []
        for b in range(num_bins):
            left, center, right = mel_low + f32(b) * delta, mel_low + f32(b + 1) * delta, mel_low + f32(b + 2) * delta
            idx = np.nonzero((mels > left) & (mels < right))[0]
            if len(idx) == 0:
                raise KhError("You may have set --num-mel-bins too large.")
            m = mels[idx[0]:idx[-1] + 1]
            wts = np.where(m <= center, (m - left) / (center - left), (right - m) / (right - center)).astype(np.float32)
            wts[~((m > left) & (m < right))] = 0.0
            first.append(int(idx[0]))
            weights.append(wts)
            off.append(off[-1] + len(wts))
        self.mel_first = np.asarray(first, np.int32)
        self.mel_off = np.asarray(off, np.int32)
        self.mel_weights = np.concatenate(weights).astype(np.float32)
        # ComputeDctMatrix matrix-functions.cc:592-608 (first num_ceps rows)
        N = num_bins
        dct = np.empty((num_ceps, N), np.float32)
        dct[0] = f32(np.sqrt(1.0 / float(f32(N))))
        norm = f32(np.sqrt(2.0 / float(f32(N))))
        k = np.arange(1, num_ceps)[:, None]
        nn = np.arange(N)[None, :]
        dct[1:] = (float(norm) * np.cos(np.pi / N * (nn + 0.5) * k)).astype(np.float32)
        self.dct = np.ascontiguousarray(dct)
        self.lifter = None
        if cepstral_lifter != 0.0:                                                      # mel-computations.cc:248-254
            q = float(f32(cepstral_lifter))
            self.lifter = (1.0 + 0.5 * q * np.sin(np.pi * np.arange(num_ceps) / q)).astype(np.float32)

    def num_frames(self, n_samples):
        """NumFrames feature-functions.cc:29-48."""
        if not self.opts.snip_edges:
            return int(np.float32(n_samples) * np.float32(1.0) / np.float32(self.frame_shift) + np.float32(0.5))
        return 0 if n_samples < self.frame_length else 1 + (n_samples - self.frame_length) // self.frame_shift

    def compute(self, wave):
        """Mfcc::Compute(wave, 1.0, &output): wave = 1-D float32 device tensor."""
        rows = self.num_frames(wave.numel())
        stride = (self.num_ceps + 3) // 4 * 4
        out = torch.empty((max(rows, 1), stride), dtype=torch.float32, device=wave.device)[:rows, :self.num_ceps]
        nf = C.c_int32()
        fp, ip = capi.c_float_p, capi.c_int32_p
        check(lib().kh_mfcc_compute_opts(
            C.c_void_p(wave.data_ptr()), wave.numel(), self.frame_shift, self.frame_length, self.padded, self.preemph,
            int(self.remove_dc), self.window.ctypes.data_as(fp), self.num_bins, self.mel_first.ctypes.data_as(ip),
            self.mel_off.ctypes.data_as(ip), self.mel_weights.ctypes.data_as(fp), self.num_ceps,
            self.dct.ctypes.data_as(fp), self.lifter.ctypes.data_as(fp) if self.lifter is not None else None,
            C.byref(self.opts), C.c_void_p(out.data_ptr()) if rows else None, stride, C.byref(nf)))
        assert nf.value == rows
        return out


def delta_scales(order, window):
    """DeltaFeatures::DeltaFeatures feat/feature-functions.cc:210-242."""
    scales = [np.ones(1, np.float32)]
    for _ in range(order):
        prev = scales[-1]
        prev_offset = (len(prev) - 1) // 2
        cur = np.zeros(len(prev) + 2 * window, np.float32)
        normalizer = np.float32(0.0)
        for j in range(-window, window + 1):
            normalizer = np.float32(normalizer + np.float32(j * j))
            for k in range(-prev_offset, prev_offset + 1):
                cur[j + k + prev_offset + window] = np.float32(cur[j + k + prev_offset + window] + np.float32(j) * prev[k + prev_offset])
        scales.append((cur * np.float32(1.0 / float(normalizer))).astype(np.float32))
    return scales


def compute_deltas(feats, order=2, window=2):
    """ComputeDeltas (feat/feature-functions.cc:361-372): feats [T x D] device -> [T x D(order+1)]."""
    if not (0 <= order < 1000 and 0 < window < 1000):
        raise KhError("DeltaFeaturesOptions: bad order / window")
    sc = delta_scales(order, window)
    flat = np.ascontiguousarray(np.concatenate(sc), np.float32)
    lens = np.ascontiguousarray([len(x) for x in sc], np.int32)
    cols = feats.shape[1] * (order + 1)
    stride = (cols + 3) // 4 * 4
    out = torch.empty((feats.shape[0], stride), dtype=torch.float32, device=feats.device)[:, :cols]
    check(lib().kh_compute_deltas(_p(feats), _dim(feats), int(order), flat.ctypes.data_as(capi.c_float_p),
                                  lens.ctypes.data_as(capi.c_int32_p), _p(out), stride))
    return out


def acc_cmvn_stats(feats, stats=None):
    """AccCmvnStats (transform/cmvn.cc:49-62): stats [2 x (dim + 1)] float64 on the host."""
    st = np.zeros((2, feats.shape[1] + 1)) if stats is None else np.ascontiguousarray(stats, np.float64)
    check(lib().kh_acc_cmvn_stats(_p(feats), _dim(feats), st.ctypes.data_as(capi.c_double_p)))
    return st


def apply_cmvn(stats, var_norm, feats):
    """ApplyCmvn (transform/cmvn.cc:64-113), in place on the device matrix."""
    dim = stats.shape[1] - 1
    if stats.shape[0] not in (1, 2) or feats.shape[1] != dim:
        raise KhError("Dim mismatch: cmvn %dx%d, feats %dx%d" % (stats.shape + tuple(feats.shape)))
    if stats.shape[0] == 1 and var_norm:
        raise KhError("You requested variance normalization but no variance stats are supplied.")
    count = float(stats[0, dim])
    if count < 1.0:
        raise KhError("Insufficient stats for cepstral mean and variance normalization: count = %g" % count)
    mean = stats[0, :dim] / count
    if not var_norm:
        scale, offset = np.ones(dim), -mean
    else:
        var = np.maximum(stats[1, :dim] / count - mean * mean, 1.0e-20)
        scale = 1.0 / np.sqrt(var)
        offset = -(mean * scale)
    dev = feats.device
    if var_norm:
        mul_cols_vec(feats, torch.from_numpy(scale.astype(np.float32)).to(dev))
    add_vec_to_rows(feats, 1.0, torch.from_numpy(offset.astype(np.float32)).to(dev))
    return feats


# ---------------------------------------------------------------- DiagGmm
def gmm_compute_gconsts(weights, means_invvars, inv_vars):
    """DiagGmm::ComputeGconsts (gmm/diag-gmm.cc:114-152); host arrays."""
    w = np.ascontiguousarray(weights, np.float32)
    mi = np.ascontiguousarray(means_invvars, np.float32)
    iv = np.ascontiguousarray(inv_vars, np.float32)
    g = np.empty(len(w), np.float32)
    fp = capi.c_float_p
    rc = lib().kh_gmm_compute_gconsts(w.ctypes.data_as(fp), mi.ctypes.data_as(fp), iv.ctypes.data_as(fp),
                                      mi.shape[0], mi.shape[1], g.ctypes.data_as(fp))
    if rc < 0:
        check(rc)
    return g, rc


class AmDiagGmm:
    """All pdfs' DiagGmm parameters concatenated, resident on the device
    (AmDiagGmm gmm/am-diag-gmm.h; scoring as DecodableAmDiagGmmUnmapped)."""

    def __init__(self, gconsts, means_invvars, inv_vars, pdf_offsets, device="cuda"):
        self.gconsts = torch.as_tensor(np.ascontiguousarray(gconsts, np.float32), device=device)
        self.means_invvars = torch.as_tensor(np.ascontiguousarray(means_invvars, np.float32), device=device)
        self.inv_vars = torch.as_tensor(np.ascontiguousarray(inv_vars, np.float32), device=device)
        self.pdf_offsets = torch.as_tensor(np.ascontiguousarray(pdf_offsets, np.int32), device=device)
        self.num_mix = self.means_invvars.shape[0]
        self.dim = self.means_invvars.shape[1]
        self.num_pdfs = self.pdf_offsets.numel() - 1

    def log_likelihoods(self, data, out=None):
        """DiagGmm::LogLikelihoods(Matrix) (diag-gmm.cc:546-562) over ALL Gaussians: T x M."""
        if data.shape[0] == 0:
            raise KhError("KALDI_ASSERT: data.NumRows() != 0")
        if data.shape[1] != self.dim:
            raise KhError("DiagGmm::ComponentLogLikelihood, dimension mismatch %d vs. %d" % (data.shape[1], self.dim))
        if out is None:
            out = torch.empty((data.shape[0], self.num_mix), dtype=torch.float32, device=data.device)
        check(lib().kh_diag_gmm_loglikes(_p(data), _dim(data), _p(self.gconsts), _p(self.means_invvars),
                                         _p(self.inv_vars), self.num_mix, _p(out), _dim(out).stride))
        return out

    def pdf_log_likelihoods(self, data, log_sum_exp_prune=-1.0, out=None):
        """frame x pdf matrix (gmm-compute-likes.cc:70-77)."""
        if data.shape[0] == 0:
            raise KhError("KALDI_ASSERT: data.NumRows() != 0")
        if data.shape[1] != self.dim:
            raise KhError("Dim mismatch: data dim = %d vs. model dim = %d" % (data.shape[1], self.dim))
        if out is None:
            out = torch.empty((data.shape[0], self.num_pdfs), dtype=torch.float32, device=data.device)
        check(lib().kh_am_gmm_loglikes(_p(data), _dim(data), _p(self.gconsts), _p(self.means_invvars),
                                       _p(self.inv_vars), _p(self.pdf_offsets), self.num_pdfs, self.num_mix,
                                       float(log_sum_exp_prune), _p(out), _dim(out).stride))
        return out


# ---------------------------------------------------------------- decoder
def decoder_config(beam=16.0, max_active=2147483647, min_active=200, lattice_beam=10.0,
                   prune_interval=25, beam_delta=0.5, hash_ratio=2.0, prune_scale=0.1):
    """LatticeFasterDecoderConfig with the reference's defaults
    (decoder/lattice-faster-decoder.h:58-66)."""
    return dict(beam=beam, max_active=max_active, min_active=min_active, lattice_beam=lattice_beam,
                prune_interval=prune_interval, beam_delta=beam_delta, hash_ratio=hash_ratio,
                prune_scale=prune_scale)


class Fst:
    """fst::Fst<StdArc> (HCLG) resident on the device as CSR."""

    def __init__(self, graph):
        off = np.ascontiguousarray(graph["arc_offsets"], np.int64)
        il = np.ascontiguousarray(graph["ilabel"], np.int32)
        ol = np.ascontiguousarray(graph["olabel"], np.int32)
        w = np.ascontiguousarray(graph["weight"], np.float32)
        ns = np.ascontiguousarray(graph["nextstate"], np.int32)
        fin = np.ascontiguousarray(graph["final"], np.float32)
        h = lib().kh_fst_create(int(graph["num_states"]), int(graph["start"]),
                                off.ctypes.data_as(capi.c_int64_p), il.ctypes.data_as(capi.c_int32_p),
                                ol.ctypes.data_as(capi.c_int32_p), w.ctypes.data_as(capi.c_float_p),
                                ns.ctypes.data_as(capi.c_int32_p), fin.ctypes.data_as(capi.c_float_p))
        if not h:
            raise KhError(lib().kh_last_error().decode())
        self._h = C.c_void_p(h)
        self.tid2pdf = None
        self._tid2pdf_host = None
        self._checked_cols = set()
        if graph.get("tid2pdf") is not None:
            self._tid2pdf_host = np.ascontiguousarray(graph["tid2pdf"], np.int32)
            self.tid2pdf = torch.as_tensor(self._tid2pdf_host, device="cuda")

    def check_pdf_map(self, num_cols):
        """Every transition-id of the graph maps to a column of the log-likelihood matrix
        (checked once per matrix width; KhError otherwise)."""
        if num_cols in self._checked_cols:
            return
        h = self._tid2pdf_host
        check(lib().kh_fst_check_pdf_map(self._h, h.ctypes.data_as(capi.c_int32_p) if h is not None else None,
                                         len(h) if h is not None else 0, int(num_cols)))
        self._checked_cols.add(num_cols)

    def num_arcs(self):
        return lib().kh_fst_num_arcs(self._h)

    def __del__(self):
        try:
            if self._h:
                lib().kh_fst_destroy(self._h)
                self._h = None
        except Exception:
            pass


class LatticeFasterDecoder:
    """decoder/lattice-faster-decoder.h:96-413 for a batch of utterances.

    decode(loglikes, utt_row_offsets) == Decode(&decodable) per utterance with a
    DecodableMatrixScaledMapped-style decodable (decoder/decodable-matrix.h:33-84):
    loglikes[t, tid2pdf[ilabel]] already scaled."""

    def __init__(self, fst, config=None, max_batch=256, max_frames=4096, exact_reference_order=True):
        self.fst = fst
        cfg = decoder_config() if config is None else config
        self.cfg = KhDecoderConfig(**cfg)
        h = lib().kh_decoder_create(fst._h, C.byref(self.cfg), int(max_batch), int(max_frames))
        if not h:
            raise KhError(lib().kh_last_error().decode())
        self._h = C.c_void_p(h)
        self.n_utts = 0
        if not exact_reference_order:      # (the library's default is the reference's order)
            self.set_reference_order(False)

    def set_reference_order(self, enable):
        """True: the reference's own iteration order (running next_cutoff in HashList order, first-minimum ties, LIFO
        closure insertions: include/kaldi_hip.h kh_decoder_set_reference_order) - tokens and links are the ones
        LatticeFasterDecoder itself creates; the default.  False: the order-independent ("canonical") rule, a cheaper
        kernel whose lattices are the reference's only where no token lies between the final and the running cutoff."""
        check(lib().kh_decoder_set_reference_order(self._h, int(bool(enable))))

    def search_counters(self, utt=0):
        c = (C.c_int64 * 2)()
        check(lib().kh_decoder_get_search_counters(self._h, int(utt), c))
        return dict(candidates_materialised=int(c[0]), reference_order=bool(c[1]))

    def __del__(self):
        try:
            if self._h:
                lib().kh_decoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def decode(self, loglikes, utt_row_offsets=None):
        if utt_row_offsets is None:
            utt_row_offsets = [0, loglikes.shape[0]]
        off = np.ascontiguousarray(utt_row_offsets, np.int32)
        self.n_utts = len(off) - 1
        self._T = np.diff(off)
        t2p = _p(self.fst.tid2pdf) if self.fst.tid2pdf is not None else None
        self.fst.check_pdf_map(loglikes.shape[1])
        self._ll = loglikes  # keep alive
        check(lib().kh_decoder_decode(self._h, _p(loglikes), _dim(loglikes).stride,
                                      off.ctypes.data_as(capi.c_int32_p), self.n_utts, t2p))
        exc, self._after_exc = getattr(self, "_after_exc", None), None
        if exc is not None:
            raise exc

    def stats(self, utt=0):
        st = KhDecodeStats()
        check(lib().kh_decoder_get_stats(self._h, int(utt), C.byref(st)))
        return {k: getattr(st, k) for k, _ in KhDecodeStats._fields_}

    def counters(self, utt=0):
        st = KhDecodeStats()
        check(lib().kh_decoder_get_counters(self._h, int(utt), C.byref(st)))
        return {k: getattr(st, k) for k, _ in KhDecodeStats._fields_}

    def set_determinize(self, enable, beam=None, delta=2.0 ** -10, max_mem=50000000, tid_phone=None, phone_determinize=None,
                        word_determinize=True, minimize=False):
        """LatticeFasterDecoderConfig::determinize_lattice + det_opts (lattice-faster-decoder.h:75-91): the host
        threads that build an utterance's raw lattice while the kernel decodes the rest of the batch also run
        DeterminizeLatticePhonePrunedWrapper on it (decoder-wrappers.cc:264-274); beam defaults to the lattice beam,
        phone_determinize to the reference's default (true) when the transition model's tid_phone map is given."""
        if phone_determinize is None:
            phone_determinize = tid_phone is not None
        tp = np.ascontiguousarray(tid_phone, np.int32) if tid_phone is not None else None
        check(lib().kh_decoder_set_determinize(self._h, int(bool(enable)), float(beam if beam is not None else self.cfg.lattice_beam),
                                               float(delta), int(max_mem), tp.ctypes.data_as(capi.c_int32_p) if tp is not None else None,
                                               len(tp) if tp is not None else 0, int(bool(phone_determinize)), int(bool(word_determinize)),
                                               int(bool(minimize))))

    def get_compact_lattice(self, utt=0):
        """The utterance's determinized CompactLattice (set_determinize(True) first), determinize_lattice_pruned's layout."""
        h = lib().kh_decoder_get_compact_lattice(self._h, int(utt))
        if not h:
            raise KhError(lib().kh_last_error().decode())
        return _read_compact_lattice(C.c_void_p(h))

    def compact_lattice_totals(self):
        """States / arcs / transition-ids of the batch's CompactLattices and how many stopped at the memory limit."""
        out = (C.c_int64 * 4)()
        check(lib().kh_decoder_compact_lattice_totals(self._h, out))
        return dict(states=int(out[0]), arcs=int(out[1]), string_labels=int(out[2]), incomplete=int(out[3]))

    def schedule_counters(self, utt=0):
        """How the pruning schedule treated the utterance (include/kaldi_hip.h kh_decoder_get_schedule_counters)."""
        c = np.zeros(4, np.int32)
        check(lib().kh_decoder_get_schedule_counters(self._h, int(utt), c.ctypes.data_as(capi.c_int32_p)))
        return dict(garbage_collections=int(c[0]), dense_final_visits=int(c[1]), general_final_visits=int(c[2]),
                    handoffs_through_memory=int(c[3]))

    def last_kernel_ms(self):
        ms = C.c_float()
        check(lib().kh_decoder_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_host_tail_ms(self):
        ms = C.c_float()
        check(lib().kh_decoder_last_host_tail_ms(self._h, C.byref(ms)))
        return ms.value

    def set_after_launch(self, fn):
        """fn() is called inside decode() when its LAST decode kernel has finished (nothing on the device reads this batch's
        scores any more) and before decode() waits for its host threads, on the calling thread: the caller's turn while
        the host finishes the batch - e.g. start the next batch's forward pass, which then runs under this batch's
        determinization.  None: off.  An exception raised by fn is re-raised by decode()."""
        self._after_exc = None
        if fn is None:
            self._after_cb = None
            check(lib().kh_decoder_set_after_launch(self._h, None, None))
            return

        def tramp(_arg):
            try:
                fn()
            except BaseException as e:   # (must not propagate through the C frames)
                self._after_exc = e
        self._after_cb = C.CFUNCTYPE(None, C.c_void_p)(tramp)
        check(lib().kh_decoder_set_after_launch(self._h, C.cast(self._after_cb, C.c_void_p), None))

    def reached_final(self, utt=0):
        return bool(self.stats(utt)["reached_final"])

    def get_raw_lattice(self, utt=0):
        """GetRawLattice (lattice-faster-decoder.cc:109-191), canonical form."""
        st = self.stats(utt)
        n, m = st["num_tokens"], st["num_links"]
        L = dict(state_frame=np.empty(n, np.int32), state_hclg=np.empty(n, np.int32),
                 state_final=np.empty(n, np.float32), arc_src=np.empty(m, np.int32),
                 arc_dst=np.empty(m, np.int32), arc_il=np.empty(m, np.int32), arc_ol=np.empty(m, np.int32),
                 arc_g=np.empty(m, np.float32), arc_a=np.empty(m, np.float32))
        ip, fp = capi.c_int32_p, capi.c_float_p
        check(lib().kh_decoder_get_raw_lattice(
            self._h, int(utt), L["state_frame"].ctypes.data_as(ip), L["state_hclg"].ctypes.data_as(ip),
            L["state_final"].ctypes.data_as(fp), L["arc_src"].ctypes.data_as(ip), L["arc_dst"].ctypes.data_as(ip),
            L["arc_il"].ctypes.data_as(ip), L["arc_ol"].ctypes.data_as(ip), L["arc_g"].ctypes.data_as(fp),
            L["arc_a"].ctypes.data_as(fp)))
        return L

    def prepare(self, num_threads=0):
        """GetRawLattice + GetBestPath of every utterance of the batch on host
        threads (decoder-wrappers.cc:215-262 per utterance); 0 = all cores."""
        check(lib().kh_decoder_prepare(self._h, int(num_threads)))

    def get_best_path(self, utt=0):
        """GetBestPath + GetLinearSymbolSequence (decoder-wrappers.cc:232-246)."""
        cap = int(self._T[utt]) + 16
        capw = 4 * cap + 64
        ali, words = np.empty(cap, np.int32), np.empty(capw, np.int32)
        na, nw = C.c_int32(), C.c_int32()
        g, a = C.c_float(), C.c_float()
        check(lib().kh_decoder_get_best_path(self._h, int(utt), ali.ctypes.data_as(capi.c_int32_p), cap, C.byref(na),
                                             words.ctypes.data_as(capi.c_int32_p), capw, C.byref(nw),
                                             C.byref(g), C.byref(a)))
        return dict(alignment=ali[:na.value].copy(), words=words[:nw.value].copy(),
                    graph_cost=g.value, acoustic_cost=a.value)

    def get_best_paths(self, first=0, n=None):
        """get_best_path of utterances [first, first + n) in one call: dict of alignment / words (concatenated,
        with ali_off / words_off = n + 1 offsets), graph_cost / acoustic_cost arrays [n]."""
        n = len(self._T) - first if n is None else int(n)
        cap = int(np.sum(self._T[first:first + n])) + 16 * n + 16
        capw = 4 * cap + 64
        ali, words = np.empty(cap, np.int32), np.empty(capw, np.int32)
        ao, wo = np.empty(n + 1, np.int64), np.empty(n + 1, np.int64)
        g, a = np.empty(n, np.float32), np.empty(n, np.float32)
        i64 = C.POINTER(C.c_int64)
        check(lib().kh_decoder_get_best_paths(self._h, int(first), n, ali.ctypes.data_as(capi.c_int32_p), cap, ao.ctypes.data_as(i64),
                                              words.ctypes.data_as(capi.c_int32_p), capw, wo.ctypes.data_as(i64),
                                              g.ctypes.data_as(capi.c_float_p), a.ctypes.data_as(capi.c_float_p)))
        return dict(alignment=ali[:ao[n]], ali_off=ao, words=words[:wo[n]], words_off=wo, graph_cost=g, acoustic_cost=a)

    def stats_batch(self, first=0, n=None, counters=True, stats=True):
        """counters(u) / stats(u) of utterances [first, first + n) in one call: two structured arrays (or None)."""
        n = len(self._T) - first if n is None else int(n)
        ca = (KhDecodeStats * n)() if counters else None
        sa = (KhDecodeStats * n)() if stats else None
        check(lib().kh_decoder_get_stats_batch(self._h, int(first), n, ca, sa))
        as_np = lambda arr: None if arr is None else np.ctypeslib.as_array(arr)
        return as_np(ca), as_np(sa)


class LatticeFasterOnlineDecoder:
    """decoder/lattice-faster-online-decoder.h:44-200 for num_streams concurrent
    utterances: InitDecoding / AdvanceDecoding (a chunk of frames at a time) /
    FinalizeDecoding, GetRawLattice and GetBestPath at any point.  The scaled
    log-likelihood chunks are what DecodableNnet2Online would serve for the next
    frames (rows [t, t + n) of the utterance's matrix)."""

    def __init__(self, fst, config=None, num_streams=1, max_frames=4096, exact_reference_order=True):
        self.fst = fst
        cfg = decoder_config() if config is None else config
        self.cfg = KhDecoderConfig(**cfg)
        self.num_streams = int(num_streams)
        h = lib().kh_online_decoder_create(fst._h, C.byref(self.cfg), self.num_streams, int(max_frames))
        if not h:
            raise KhError(lib().kh_last_error().decode())
        self._h = C.c_void_p(h)
        if not exact_reference_order:      # (the library's default is the reference's order)
            self.set_reference_order(False)

    def __del__(self):
        try:
            if self._h:
                lib().kh_online_decoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @staticmethod
    def _streams(streams):
        a = np.ascontiguousarray(streams, np.int32).reshape(-1)
        return a, a.ctypes.data_as(capi.c_int32_p), len(a)

    def init_decoding(self, streams):
        a, ptr, n = self._streams(streams)
        check(lib().kh_online_decoder_init_decoding(self._h, ptr, n))

    def advance_decoding(self, streams, chunks):
        """chunks[i]: 2-D float32 device tensor, the next rows of stream streams[i]
        (all with the same row stride)."""
        a, ptr, n = self._streams(streams)
        assert len(chunks) == n
        strides = {int(_dim(c).stride) for c in chunks if c.shape[0] > 0}
        assert len(strides) <= 1, "chunks of one call must share their row stride"
        stride = strides.pop() if strides else 1
        ptrs = (C.c_void_p * n)(*[C.c_void_p(c.data_ptr()) if c.shape[0] > 0 else None for c in chunks])
        nf = np.ascontiguousarray([c.shape[0] for c in chunks], np.int32)
        t2p = _p(self.fst.tid2pdf) if self.fst.tid2pdf is not None else None
        for c in chunks:
            if c.shape[0] > 0:
                self.fst.check_pdf_map(c.shape[1])
        self._keep = chunks
        check(lib().kh_online_decoder_advance(self._h, ptr, n, ptrs, stride, nf.ctypes.data_as(capi.c_int32_p), t2p))

    def set_lazy_prune(self, enable=True):
        """The offline kernel's lazy pruning schedule (kh_online_decoder_set_lazy_prune): same final lattices and best paths,
        no pruning while the streams advance; every stream must be idle."""
        check(lib().kh_online_decoder_set_lazy_prune(self._h, int(bool(enable))))

    def set_reference_order(self, enable=True):
        """The reference's own iteration order for the streams (kh_online_decoder_set_reference_order;
        lattice-faster-online-decoder.cc:864-951): the lattices LatticeFasterOnlineDecoder itself would build; the default.
        Every stream must be idle and the persistent serving kernel stopped while switching; a serving kernel started
        afterwards decodes in the same order (ServeKernel<kExact>)."""
        check(lib().kh_online_decoder_set_reference_order(self._h, int(bool(enable))))

    def num_frames_decoded(self, stream=0):
        n = C.c_int32()
        check(lib().kh_online_decoder_num_frames_decoded(self._h, int(stream), C.byref(n)))
        return n.value

    def finalize_decoding(self, streams):
        a, ptr, n = self._streams(streams)
        check(lib().kh_online_decoder_finalize(self._h, ptr, n))

    def stats(self, stream=0, use_final_probs=True):
        st = KhDecodeStats()
        check(lib().kh_online_decoder_get_stats(self._h, int(stream), int(bool(use_final_probs)), C.byref(st)))
        return {k: getattr(st, k) for k, _ in KhDecodeStats._fields_}

    def get_raw_lattice(self, stream=0, use_final_probs=True):
        st = self.stats(stream, use_final_probs)
        n, m = st["num_tokens"], st["num_links"]
        L = dict(state_frame=np.empty(n, np.int32), state_hclg=np.empty(n, np.int32),
                 state_final=np.empty(n, np.float32), arc_src=np.empty(m, np.int32),
                 arc_dst=np.empty(m, np.int32), arc_il=np.empty(m, np.int32), arc_ol=np.empty(m, np.int32),
                 arc_g=np.empty(m, np.float32), arc_a=np.empty(m, np.float32))
        i32 = lambda k: L[k].ctypes.data_as(capi.c_int32_p)
        f32 = lambda k: L[k].ctypes.data_as(capi.c_float_p)
        check(lib().kh_online_decoder_get_raw_lattice(
            self._h, int(stream), int(bool(use_final_probs)), i32("state_frame"), i32("state_hclg"),
            f32("state_final"), i32("arc_src"), i32("arc_dst"), i32("arc_il"), i32("arc_ol"), f32("arc_g"), f32("arc_a")))
        return L

    def get_best_path(self, stream=0, use_final_probs=True):
        cap = self.num_frames_decoded(stream) + 16
        capw = 4 * cap + 64
        ali, words = np.empty(cap, np.int32), np.empty(capw, np.int32)
        na, nw = C.c_int32(), C.c_int32()
        g, a = C.c_float(), C.c_float()
        check(lib().kh_online_decoder_get_best_path(
            self._h, int(stream), int(bool(use_final_probs)), ali.ctypes.data_as(capi.c_int32_p), cap, C.byref(na),
            words.ctypes.data_as(capi.c_int32_p), capw, C.byref(nw), C.byref(g), C.byref(a)))
        return dict(alignment=ali[:na.value].copy(), words=words[:nw.value].copy(),
                    graph_cost=g.value, acoustic_cost=a.value)


# ---------------------------------------------------------------- lattice forward-backward
def lattice_to_csr(L):
    """Raw lattice (get_raw_lattice: states in canonical (frame, HCLG state) order, start first)
    -> top-sorted CSR, the form LatticeForwardBackward needs (the reference top-sorts lattices
    it reads: TopSortLatticeIfNeeded, lat/lattice-functions.cc, before
    nnet-compute-discriminative.cc:178).  Epsilon arcs may point backwards in the canonical
    order, so states are ordered by (frame, epsilon depth, state)."""
    n = len(L["state_frame"])
    depth = np.zeros(n, np.int64)
    eps = L["arc_il"] == 0
    es, ed = L["arc_src"][eps], L["arc_dst"][eps]
    for _ in range(n + 1):
        nd = depth.copy()
        np.maximum.at(nd, ed, depth[es] + 1)
        if np.array_equal(nd, depth):
            break
        depth = nd
    order = np.lexsort((L["state_hclg"], depth, L["state_frame"]))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    src, dst = rank[L["arc_src"]], rank[L["arc_dst"]]
    perm = np.lexsort((np.arange(len(src)), src))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(src, minlength=n))
    return dict(n_states=n, arc_offsets=off, arc_ilabel=L["arc_il"][perm].astype(np.int32),
                arc_nextstate=dst[perm].astype(np.int32), arc_graph=L["arc_g"][perm].astype(np.float32),
                arc_acoustic=L["arc_a"][perm].astype(np.float32),
                state_final=L["state_final"][order].astype(np.float32), perm=perm, order=order)


def lattice_forward_backward(lats):
    """LatticeForwardBackward (lat/lattice-functions.cc:272-354) for a batch of
    top-sorted lattices.  Each lattice is a dict with n_states, arc_offsets (int64,
    n_states+1), arc_ilabel, arc_nextstate, arc_graph, arc_acoustic, state_final.
    Returns per lattice: dict(arc_post, tot_like, acoustic_like_sum, state_times, post)
    where post is the Posterior: per frame a sorted list of (transition-id, weight)
    merged as MergePairVectorSumming does (:351-352)."""
    n = len(lats)
    soff = np.zeros(n + 1, np.int32)
    for i, L in enumerate(lats):
        soff[i + 1] = soff[i] + L["n_states"]
    aoff = [np.zeros(1, np.int64)]
    base = 0
    for L in lats:
        o = np.asarray(L["arc_offsets"], np.int64)
        aoff.append(o[1:] + base)
        base += int(o[-1])
    aoff = np.ascontiguousarray(np.concatenate(aoff))
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(L[k], dt) for L in lats]))
    il, ns = cat("arc_ilabel", np.int32), cat("arc_nextstate", np.int32)
    g, a, fin = cat("arc_graph", np.float32), cat("arc_acoustic", np.float32), cat("state_final", np.float32)
    post = np.empty(len(il), np.float32)
    tot, ac = np.empty(n, np.float64), np.empty(n, np.float64)
    times = np.empty(int(soff[-1]), np.int32)
    ip, fp, dp = capi.c_int32_p, capi.c_float_p, capi.c_double_p
    check(lib().kh_lattice_forward_backward(
        n, soff.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), il.ctypes.data_as(ip),
        ns.ctypes.data_as(ip), g.ctypes.data_as(fp), a.ctypes.data_as(fp), fin.ctypes.data_as(fp),
        post.ctypes.data_as(fp), tot.ctypes.data_as(dp), ac.ctypes.data_as(dp), times.ctypes.data_as(ip)))
    out = []
    for i, L in enumerate(lats):
        a0, a1 = int(aoff[soff[i]]), int(aoff[soff[i + 1]])
        t = times[soff[i]:soff[i + 1]]
        ap = post[a0:a1]
        max_time = int(t.max()) if len(t) else 0
        posterior = _arc_posterior_to_post(L, t, il[a0:a1], ap, max_time)
        out.append(dict(arc_post=ap.copy(), tot_like=float(tot[i]), acoustic_like_sum=float(ac[i]),
                        state_times=t.copy(), post=posterior))
    return out


def _cat_lattices(lats):
    n = len(lats)
    soff = np.zeros(n + 1, np.int32)
    for i, L in enumerate(lats):
        soff[i + 1] = soff[i] + L["n_states"]
    aoff = [np.zeros(1, np.int64)]
    base = 0
    for L in lats:
        o = np.asarray(L["arc_offsets"], np.int64)
        aoff.append(o[1:] + base)
        base += int(o[-1])
    aoff = np.ascontiguousarray(np.concatenate(aoff))
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(L[k], dt) for L in lats]))
    return (n, soff, aoff, cat("arc_ilabel", np.int32), cat("arc_nextstate", np.int32), cat("arc_graph", np.float32),
            cat("arc_acoustic", np.float32), cat("state_final", np.float32))


def _arc_posterior_to_post(L, times, tids, arc_post, max_time):
    """(*post)[state_times[s]].push_back((tid, p)) for tid != 0, then MergePairVectorSumming
    (util/stl-utils.h: sort by tid, sum equal keys in float in their original order, drop
    zeros).  Vectorised: stable sort by (frame, tid), sequential float32 sums (np.add.at)."""
    src = np.repeat(np.arange(L["n_states"]), np.diff(np.asarray(L["arc_offsets"], np.int64)))
    m = tids != 0
    fr, ti, p = times[src[m]].astype(np.int64), tids[m].astype(np.int64), arc_post[m].astype(np.float32)
    key = fr * (int(ti.max()) + 1 if len(ti) else 1) + ti
    order = np.argsort(key, kind="stable")
    key, fr, ti, p = key[order], fr[order], ti[order], p[order]
    first = np.ones(len(key), bool)
    first[1:] = key[1:] != key[:-1]
    grp = np.cumsum(first) - 1
    acc = np.zeros(int(grp[-1]) + 1 if len(grp) else 0, np.float32)
    np.add.at(acc, grp, p)                       # unbuffered: adds in array order
    gfr, gti = fr[first], ti[first]
    keep = acc != 0.0
    gfr, gti, acc = gfr[keep], gti[keep], acc[keep]
    bounds = np.searchsorted(gfr, np.arange(max_time + 1))
    tl, wl = gti.tolist(), acc.tolist()
    return [list(zip(tl[bounds[t]:bounds[t + 1]], wl[bounds[t]:bounds[t + 1]])) for t in range(max_time)]


def lattice_alphas_betas(lats, viterbi=False):
    """ComputeLatticeAlphasAndBetas (lat/lattice-functions.cc:412-463) for a batch."""
    n, soff, aoff, il, ns, g, a, fin = _cat_lattices(lats)
    alpha, beta, tot = np.empty(int(soff[-1])), np.empty(int(soff[-1])), np.empty(n)
    ip, fp, dp = capi.c_int32_p, capi.c_float_p, capi.c_double_p
    check(lib().kh_lattice_alphas_betas(
        n, soff.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), il.ctypes.data_as(ip), ns.ctypes.data_as(ip),
        g.ctypes.data_as(fp), a.ctypes.data_as(fp), fin.ctypes.data_as(fp), int(bool(viterbi)),
        alpha.ctypes.data_as(dp), beta.ctypes.data_as(dp), tot.ctypes.data_as(dp)))
    return [dict(alpha=alpha[soff[i]:soff[i + 1]].copy(), beta=beta[soff[i]:soff[i + 1]].copy(), tot=float(tot[i]))
            for i in range(n)]


def lattice_forward_backward_mpe(lats, tid2phone, tid2pdf, silence_phones, num_alis, criterion="smbr",
                                 one_silence_class=False):
    """LatticeForwardBackwardMpeVariants (lat/lattice-functions.cc:740-919) for a batch;
    returns per lattice dict(arc_post, post, tot_forward_score)."""
    if criterion not in ("smbr", "mpfe"):
        raise KhError('criterion must be "mpfe" or "smbr" (lattice-functions.cc:753)')
    n, soff, aoff, il, ns, g, a, fin = _cat_lattices(lats)
    t2ph, t2pdf = np.ascontiguousarray(tid2phone, np.int32), np.ascontiguousarray(tid2pdf, np.int32)
    sil = np.ascontiguousarray(sorted(silence_phones), np.int32)
    ali_off = np.concatenate([[0], np.cumsum([len(x) for x in num_alis])]).astype(np.int32)
    ali = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in num_alis]) if len(num_alis) else [], np.int32)
    post = np.empty(len(il), np.float32)
    score = np.empty(n)
    all_times = np.empty(int(soff[-1]), np.int32)
    ip, fp, dp = capi.c_int32_p, capi.c_float_p, capi.c_double_p
    check(lib().kh_lattice_forward_backward_mpe(
        n, soff.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), il.ctypes.data_as(ip), ns.ctypes.data_as(ip),
        g.ctypes.data_as(fp), a.ctypes.data_as(fp), fin.ctypes.data_as(fp), t2ph.ctypes.data_as(ip),
        t2pdf.ctypes.data_as(ip), len(t2ph) - 1, sil.ctypes.data_as(ip), len(sil), ali.ctypes.data_as(ip),
        ali_off.ctypes.data_as(ip), int(criterion == "mpfe"), int(bool(one_silence_class)), post.ctypes.data_as(fp),
        score.ctypes.data_as(dp), all_times.ctypes.data_as(ip)))
    out = []
    for i, L in enumerate(lats):
        a0, a1 = int(aoff[soff[i]]), int(aoff[soff[i + 1]])
        times = all_times[soff[i]:soff[i + 1]]
        out.append(dict(arc_post=post[a0:a1].copy(), tot_forward_score=float(score[i]),
                        post=_arc_posterior_to_post(L, times, il[a0:a1], post[a0:a1], len(num_alis[i]))))
    return out


def lattice_state_times(L):
    """LatticeStateTimes (lat/lattice-functions.cc:36-67) of one top-sorted lattice."""
    n = L["n_states"]
    off = np.asarray(L["arc_offsets"], np.int64)
    il, ns = np.asarray(L["arc_ilabel"]), np.asarray(L["arc_nextstate"])
    times = np.full(n, -1, np.int32)
    times[0] = 0
    for s in range(n):
        for a in range(off[s], off[s + 1]):
            want = times[s] + (1 if il[a] != 0 else 0)
            if times[ns[a]] == -1:
                times[ns[a]] = want
            elif times[ns[a]] != want:
                raise KhError("LatticeStateTimes: inconsistent lattice")
    return times


def lattice_state_times_batch(lats):
    """LatticeStateTimes of a batch on the device (kh_lattice_state_times: the preparation kernel alone, no costs uploaded):
    per lattice dict(state_times, max_time); -1 for a state no path from state 0 reaches."""
    n, soff, aoff, il, ns, _, _, fin = _cat_lattices(lats)
    times, max_times = np.empty(int(soff[-1]), np.int32), np.empty(n, np.int32)
    ip = capi.c_int32_p
    check(lib().kh_lattice_state_times(n, soff.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), il.ctypes.data_as(ip),
                                       ns.ctypes.data_as(ip), fin.ctypes.data_as(capi.c_float_p), times.ctypes.data_as(ip),
                                       max_times.ctypes.data_as(ip)))
    return [dict(state_times=times[soff[i]:soff[i + 1]].copy(), max_time=int(max_times[i])) for i in range(n)]


class LatticeBatch:
    """A batch of top-sorted lattices kept on the device (kh_lattice_batch_*): uploaded and prepared once; forward-backward,
    rescoring with a new score matrix and the forward-backward after it run from there (what
    NnetDiscriminativeUpdater::LatticeComputations does to one lattice, nnet-compute-discriminative.cc:178-321)."""

    def __init__(self, lats):
        self.n, self.soff, self.aoff, il, ns, g, a, fin = _cat_lattices(lats) if not isinstance(lats, tuple) else lats
        self._il = il
        ip, fp = capi.c_int32_p, capi.c_float_p
        h = lib().kh_lattice_batch_create(self.n, self.soff.ctypes.data_as(ip), self.aoff.ctypes.data_as(capi.c_int64_p),
                                          il.ctypes.data_as(ip), ns.ctypes.data_as(ip), g.ctypes.data_as(fp), a.ctypes.data_as(fp),
                                          fin.ctypes.data_as(fp))
        if not h:
            raise KhError(lib().kh_last_error().decode())
        self._h = C.c_void_p(h)
        self.total_arcs, self.total_states = len(il), int(self.soff[-1])

    def __del__(self):
        try:
            if self._h:
                lib().kh_lattice_batch_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def forward_backward(self, want_times=False):
        """LatticeForwardBackward of every lattice: dict(arc_post [total_arcs], tot_like [n], acoustic_like_sum [n], state_times)."""
        post = np.empty(self.total_arcs, np.float32)
        tot, ac = np.empty(self.n, np.float64), np.empty(self.n, np.float64)
        times = np.empty(self.total_states, np.int32) if want_times else None
        check(lib().kh_lattice_batch_forward_backward(self._h, post.ctypes.data_as(capi.c_float_p), tot.ctypes.data_as(capi.c_double_p),
                                                      ac.ctypes.data_as(capi.c_double_p),
                                                      times.ctypes.data_as(capi.c_int32_p) if want_times else None))
        return dict(arc_post=post, tot_like=tot, acoustic_like_sum=ac, state_times=times)

    def forward_backward_device(self, out=None):
        """The same with the arc posteriors left on the device: dict(arc_post = torch tensor [total_arcs] on the GPU, tot_like,
        acoustic_like_sum)."""
        import torch
        if out is None:
            out = torch.empty(self.total_arcs, dtype=torch.float32, device="cuda")
        tot, ac = np.empty(self.n, np.float64), np.empty(self.n, np.float64)
        check(lib().kh_lattice_batch_forward_backward_dev(self._h, _p(out), tot.ctypes.data_as(capi.c_double_p),
                                                          ac.ctypes.data_as(capi.c_double_p)))
        return dict(arc_post=out, tot_like=tot, acoustic_like_sum=ac)

    def rescore(self, loglikes, utt_row_offsets, tid2pdf=None, fetch=False):
        """RescoreLattice with a device score matrix; the acoustic costs change on the device (fetch: return them)."""
        off = np.ascontiguousarray(utt_row_offsets, np.int32)
        out = np.empty(self.total_arcs, np.float32) if fetch else None
        check(lib().kh_lattice_batch_rescore(self._h, _p(loglikes), _dim(loglikes).stride, off.ctypes.data_as(capi.c_int32_p),
                                             _p(tid2pdf) if tid2pdf is not None else None,
                                             out.ctypes.data_as(capi.c_float_p) if fetch else None))
        return out


def lattice_last_timings():
    """Milliseconds the last lattice call of this thread spent in upload / device preparation / sweeps / download."""
    ms = (C.c_float * 4)()
    check(lib().kh_lattice_last_timings(ms))
    return dict(upload_ms=ms[0], prep_ms=ms[1], sweeps_ms=ms[2], download_ms=ms[3])


_LATTICE_PLAN_FIELDS = ("cus", "prep_dataflow", "prep_per_cu", "prep_win", "prep_lds_states", "n_prep_off_lds",
                        "sweep_dataflow", "sweep_per_cu", "sweep_stage", "sweep_win", "n_tagged")


def lattice_last_plan():
    """Which forms of the lattice kernels the last lattice call of this thread ran (kh_lattice_last_plan; the sizing is
    csrc/kh_lattice_plan.h): the preparation (dataflow or levels, workgroups per CU, state-time window, states whose counters
    stay in LDS, lattices above that) and the forward-backward sweep (1 dataflow / 0 levels / -1 none, workgroups per CU,
    staged arcs per wave, window slots, lattices in the tagged form)."""
    out = np.zeros(12, np.int32)
    check(lib().kh_lattice_last_plan(out.ctypes.data_as(capi.c_int32_p)))
    return {k: int(v) for k, v in zip(_LATTICE_PLAN_FIELDS, out)}


# ---------------------------------------------------------------- best paths over score points (csrc/kh_latbest.hip)
def score_point(lm_scale=1.0, acoustic_scale=1.0, inv_acoustic_scale=1.0, acoustic2lm_scale=0.0, lm2acoustic_scale=0.0,
                word_ins_penalty=0.0):
    """What `lattice-scale [options] | lattice-add-penalty --word-ins-penalty=...` do to a weight, as the pair
    (scale [4 doubles: lm, acoustic2lm, lm2acoustic, acoustic], penalty [float32]) compact_lattice_best_paths takes.  The
    options are BaseFloat = float; with inv_acoustic_scale != 1 the acoustic scale is the FLOAT quotient 1.0 / inv
    (latbin/lattice-scale.cc:72-82)."""
    ac, inv = np.float32(acoustic_scale), np.float32(inv_acoustic_scale)
    if not (ac == np.float32(1.0) or inv == np.float32(1.0)):       # KALDI_ASSERT :72
        raise KhError("score_point: acoustic_scale == 1.0 || inv_acoustic_scale == 1.0")
    if inv != np.float32(1.0):
        ac = np.float32(1.0) / inv
    scale = np.array([np.float32(lm_scale), np.float32(acoustic2lm_scale), np.float32(lm2acoustic_scale), ac], np.float64)
    return scale, np.float32(word_ins_penalty)


def compact_lattice_top_order(clat):
    """The state numbering CompactLatticeShortestPath searches in (lat/lattice-functions.cc:1046-1052): None when the
    lattice has the kTopSorted property (start state 0 and every arc to a higher-numbered state), else order[old] = new of
    fst::TopSort (fst/topsort.h): reverse finishing order of a depth-first search from the start state, then from every
    still unvisited state in number order, a state's arcs in order.  The numbering decides ties, so any other
    topological order will not do.  Raises on a cycle (:1048-1049)."""
    n = int(clat["n_states"])
    start = int(clat.get("start", 0))
    src, dst = np.asarray(clat["arc_src"], np.int64), np.asarray(clat["arc_dst"], np.int64)
    if n == 0 or start < 0:         # no start state (:1055: the best path is empty); nothing to number
        return None
    if start >= n:
        raise KhError("compact lattice: start state %d of %d states" % (start, n))
    if start == 0 and bool(np.all(dst > src)):
        return None
    by_src = np.argsort(src, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    nxt = dst[by_src].tolist()
    off = off.tolist()
    color = [0] * n          # white / grey / black
    finish = []
    for root in [start] + list(range(n)):
        if color[root]:
            continue
        color[root] = 1
        stack = [(root, off[root])]
        while stack:
            s, k = stack[-1]
            if k < off[s + 1]:
                stack[-1] = (s, k + 1)
                t = nxt[k]
                if color[t] == 0:
                    color[t] = 1
                    stack.append((t, off[t]))
                elif color[t] == 1:
                    raise KhError("Was not able to topologically sort lattice (cycles found?)")
            else:
                color[s] = 2
                finish.append(s)
                stack.pop()
    order = np.empty(n, np.int64)
    order[np.asarray(finish[::-1], np.int64)] = np.arange(n)
    return order


def _clat_to_csr(clat, order):
    """The CSR dict of a CompactLattice dict in the numbering order[old] = new (None = as it is), and the start state there."""
    n = int(clat["n_states"])
    src, dst = np.asarray(clat["arc_src"], np.int64), np.asarray(clat["arc_dst"], np.int64)
    state_of = np.arange(n, dtype=np.int64)
    start = int(clat.get("start", 0))
    if order is not None:
        src, dst = order[src], order[dst]
        state_of = np.argsort(order)
        start = int(order[start])
    perm = np.argsort(src, kind="stable")
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(src, minlength=n))
    L = dict(n_states=n, arc_offsets=off, arc_label=np.asarray(clat["arc_label"], np.int32)[perm],
             arc_nextstate=dst[perm].astype(np.int32), arc_graph=np.asarray(clat["arc_g"], np.float32)[perm],
             arc_acoustic=np.asarray(clat["arc_a"], np.float32)[perm],
             final_graph=np.asarray(clat["final_g"], np.float32)[state_of],
             final_acoustic=np.asarray(clat["final_a"], np.float32)[state_of], perm=perm, state_of=state_of)
    return L, start


def compact_lattice_to_csr(clat):
    """CompactLattice dict (kaldi_io.read_compact_lattice / determinize_lattice_pruned) -> the top-sorted CSR arrays of
    kh_compact_lattice_best_paths, renumbered by compact_lattice_top_order when needed.  perm[j] = the dict's arc behind
    CSR arc j, state_of[s] = the dict's state behind CSR state s."""
    return _clat_to_csr(clat, compact_lattice_top_order(clat))[0]


# ---------------------------------------------------------------- what the batched compact-lattice calls share
def _batch_csr(csrs):
    """CSR dicts -> (soff [n + 1 int32: the first state of each lattice], aoff [states + 1 int64: the batch's arc offsets],
    lat_arc_off [n + 1 int64: the first arc of each lattice], cat): cat(key, dtype) joins that array of every dict, flattened
    (an empty array where there is nothing to join)."""
    n = len(csrs)
    soff = np.zeros(n + 1, np.int32)
    soff[1:] = np.cumsum([int(L["n_states"]) for L in csrs])
    aoff, lat_arc_off = [np.zeros(1, np.int64)], np.zeros(n + 1, np.int64)
    for i, L in enumerate(csrs):
        o = np.asarray(L["arc_offsets"], np.int64)
        aoff.append(o[1:] + lat_arc_off[i])
        lat_arc_off[i + 1] = lat_arc_off[i] + int(o[-1])
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(L[k], dt).reshape(-1) for L in csrs] + [np.zeros(0, dt)]))
    return soff, np.ascontiguousarray(np.concatenate(aoff)), lat_arc_off, cat


def _point_arrays(points):
    """[(scale, penalty)] as score_point returns them -> (scales [K x 4 float64], penalties [K float32])."""
    scales = np.ascontiguousarray(np.stack([np.asarray(s, np.float64).reshape(4) for s, _ in points]))
    return scales, np.ascontiguousarray(np.asarray([p for _, p in points], np.float32))


def _path_room(soff, K):
    """Offsets of the room for one path per (lattice, point): a path has at most n_states - 1 arcs."""
    room = np.repeat(np.maximum(np.diff(soff).astype(np.int64) - 1, 1), K)
    poff = np.zeros(len(room) + 1, np.int64)
    poff[1:] = np.cumsum(room)
    return poff


def _split_paths(parcs, poff, plen, n, K):
    return [[parcs[poff[i * K + p]:poff[i * K + p] + max(int(plen[i * K + p]), 0)].copy() for p in range(K)] for i in range(n)]


@contextlib.contextmanager
def _workspace_limit(setter, nbytes):
    """Bound the calling thread's workspace for the calls inside (None = leave the default), and set it back after."""
    if nbytes is not None:
        check(setter(int(nbytes)))
    try:
        yield
    finally:
        if nbytes is not None:
            check(setter(0))


def _timings(fn, names, count_names):
    """A *_last_timings call as a dict: the float milliseconds under `names`, then the int32 counts under `count_names`."""
    ms = (C.c_float * len(names))()
    n = (C.c_int32 * len(count_names))()
    check(fn(ms, n))
    out = dict(zip(names, ms))
    out.update(zip(count_names, n))
    return out


_MS5 = ("host_prep_ms", "upload_ms", "kernel_ms", "download_ms", "call_ms")


def compact_lattice_best_paths_raw(csrs, points, workspace_limit=None):
    """kh_compact_lattice_best_paths on CSR dicts (compact_lattice_to_csr's layout, top-sorted).  points: a list of
    (scale, penalty) as score_point returns.  Returns (path_len [n_lats x n_points], paths [list of lists of int32 arrays:
    CSR arc numbers within the lattice], final_state, tot_graph, tot_acoustic [n_lats x n_points]).  workspace_limit
    (bytes): bound the lattices in flight for this call (None = from the free device memory; the library keeps the limit
    per thread, and it is set back before this returns)."""
    n, K = len(csrs), len(points)
    if n == 0 or K == 0:
        raise KhError("compact_lattice_best_paths: no lattices or no score points")
    soff, aoff, _, cat = _batch_csr(csrs)
    lab, ns = cat("arc_label", np.int32), cat("arc_nextstate", np.int32)
    g, a = cat("arc_graph", np.float32), cat("arc_acoustic", np.float32)
    fg, fa = cat("final_graph", np.float32), cat("final_acoustic", np.float32)
    scales, pens = _point_arrays(points)
    poff = _path_room(soff, K)
    plen, pfin = np.empty(n * K, np.int32), np.empty(n * K, np.int32)
    parcs = np.empty(int(poff[-1]), np.int32)
    tg, ta = np.empty(n * K, np.float32), np.empty(n * K, np.float32)
    ip, fp = capi.c_int32_p, capi.c_float_p
    with _workspace_limit(lib().kh_compact_lattice_best_paths_set_workspace_limit, workspace_limit):
        check(lib().kh_compact_lattice_best_paths(
            n, soff.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), lab.ctypes.data_as(ip), ns.ctypes.data_as(ip),
            g.ctypes.data_as(fp), a.ctypes.data_as(fp), fg.ctypes.data_as(fp), fa.ctypes.data_as(fp), K,
            scales.ctypes.data_as(capi.c_double_p), pens.ctypes.data_as(fp), plen.ctypes.data_as(ip), parcs.ctypes.data_as(ip),
            poff.ctypes.data_as(capi.c_int64_p), pfin.ctypes.data_as(ip), tg.ctypes.data_as(fp), ta.ctypes.data_as(fp)))
    return plen.reshape(n, K), _split_paths(parcs, poff, plen, n, K), pfin.reshape(n, K), tg.reshape(n, K), ta.reshape(n, K)


def compact_lattice_best_paths(clats, points, workspace_limit=None):
    """lattice-scale | lattice-add-penalty | lattice-best-path (CompactLatticeShortestPath, lat/lattice-functions.cc:1043-1126)
    for a batch of CompactLattices (dict layout of kaldi_io.read_compact_lattice / determinize_lattice_pruned) and a list of
    score points (score_point) in ONE device call.  Returns per lattice a list over the points of None (no path: the
    reference's "Best-path failed") or dict(words = the non-zero labels of the path's arcs, alignment = the arcs'
    transition-ids followed by the final state's (ConvertLattice + GetLinearSymbolSequence, lattice-best-path.cc:89-98),
    graph_cost, acoustic_cost = the path's weight (float32), arcs = the path as indices into the dict's arc arrays,
    final_state).  Only labels and weights go to the device; the strings are joined here."""
    has_start = [int(c["n_states"]) > 0 and int(c.get("start", 0)) >= 0 for c in clats]    # :1055: no start state, empty path
    csrs = [compact_lattice_to_csr(c) for c, ok in zip(clats, has_start) if ok]
    if not csrs:
        return [[None] * len(points) for _ in clats]
    plen, paths, pfin, tg, ta = compact_lattice_best_paths_raw(csrs, points, workspace_limit)
    empty = np.zeros(0, np.int32)
    out = []
    i = -1
    for c, ok in zip(clats, has_start):
        if not ok:
            out.append([None] * len(points))
            continue
        i += 1
        L = csrs[i]
        row = []
        for p in range(len(points)):
            if plen[i, p] < 0:
                row.append(None)
                continue
            arcs = L["perm"][paths[i][p]]
            fs = int(L["state_of"][pfin[i, p]])
            labels = np.asarray(c["arc_label"], np.int32)[arcs]
            strings = [np.asarray(c["arc_string"][j], np.int32) for j in arcs] + [np.asarray(c["final_string"][fs], np.int32)]
            row.append(dict(words=labels[labels != 0], alignment=np.concatenate(strings + [empty]).astype(np.int32),
                            graph_cost=np.float32(tg[i, p]), acoustic_cost=np.float32(ta[i, p]), arcs=arcs.astype(np.int64),
                            final_state=fs))
        out.append(row)
    return out


def compact_lattice_best_paths_last_timings():
    """Milliseconds the last compact_lattice_best_paths call of this thread spent in host preparation / upload / kernels /
    download (the allocations and the host's scatter are in none of the four), in the whole C call, and the number of
    kernel launches it took."""
    return _timings(lib().kh_compact_lattice_best_paths_last_timings, _MS5, ("launches",))


# ---------------------------------------------------------------- pruning over score points (csrc/kh_latprune.hip)
def compact_lattice_prune_order(clat):
    """The state numbering PruneLattice works in (lat/lattice-functions.cc:193-198): None when the lattice has OpenFst's
    kTopSorted property - every arc goes to a higher-numbered state, WHATEVER the start state is (:199-201 then takes
    lat->Start() and leaves the states in front of it unreachable) - else order[old] = new of fst::TopSort, as
    compact_lattice_top_order numbers.  Raises on a cycle (:194-196)."""
    n = int(clat["n_states"])
    start = int(clat.get("start", 0))
    if n == 0 or start < 0:
        return None
    if start >= n:
        raise KhError("compact lattice: start state %d of %d states" % (start, n))
    if bool(np.all(np.asarray(clat["arc_dst"], np.int64) > np.asarray(clat["arc_src"], np.int64))):
        return None
    return compact_lattice_top_order(clat)


def compact_lattice_to_prune_csr(clat):
    """compact_lattice_to_csr in compact_lattice_prune_order's numbering, plus start = the start state in that numbering."""
    L, start = _clat_to_csr(clat, compact_lattice_prune_order(clat))
    return dict(L, start=start)


def _point_beams(beams, K):
    b = np.asarray(beams, np.float32).reshape(-1)
    if b.size == 1:
        b = np.repeat(b, K)
    if b.size != K:
        raise KhError("compact_lattice_prune: %d beams for %d score points" % (b.size, K))
    return np.ascontiguousarray(b)


def compact_lattice_prune_raw(csrs, starts, points, beams, workspace_limit=None):
    """kh_compact_lattice_prune on CSR dicts (compact_lattice_to_prune_csr's layout, top-sorted), starts = the start state
    of each, points as compact_lattice_best_paths_raw takes them, beams = one float or one per point.  Returns
    dict(arc_keep, state_keep, final_keep = bool [arcs or states of the whole batch x n_points], best_final_cost
    [n_lats x n_points], state_offsets, arc_offsets = where each lattice's rows begin, and arc_keep_words, state_keep_words,
    final_keep_words = the same masks as the call wrote them: uint64 [arcs or states x ceil(n_points / 64)], bit p % 64 of
    word p / 64).  workspace_limit as compact_lattice_best_paths_raw's."""
    n, K = len(csrs), len(points)
    if n == 0 or K == 0:
        raise KhError("compact_lattice_prune: no lattices or no score points")
    soff, aoff, lat_arc_off, cat = _batch_csr(csrs)
    lab, ns = cat("arc_label", np.int32), cat("arc_nextstate", np.int32)
    g, a = cat("arc_graph", np.float32), cat("arc_acoustic", np.float32)
    fg, fa = cat("final_graph", np.float32), cat("final_acoustic", np.float32)
    st = np.ascontiguousarray(np.asarray(starts, np.int32).reshape(n))
    scales, pens = _point_arrays(points)
    bm = _point_beams(beams, K)
    S, A, W = int(soff[-1]), int(lat_arc_off[-1]), (K + 63) // 64
    akeep, skeep, fkeep = np.zeros((A, W), np.uint64), np.zeros((S, W), np.uint64), np.zeros((S, W), np.uint64)
    best = np.empty((n, K), np.float64)
    ip, fp, up = capi.c_int32_p, capi.c_float_p, capi.c_uint64_p
    with _workspace_limit(lib().kh_compact_lattice_prune_set_workspace_limit, workspace_limit):
        check(lib().kh_compact_lattice_prune(
            n, soff.ctypes.data_as(ip), st.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), lab.ctypes.data_as(ip),
            ns.ctypes.data_as(ip), g.ctypes.data_as(fp), a.ctypes.data_as(fp), fg.ctypes.data_as(fp), fa.ctypes.data_as(fp), K,
            scales.ctypes.data_as(capi.c_double_p), pens.ctypes.data_as(fp), bm.ctypes.data_as(fp), akeep.ctypes.data_as(up),
            skeep.ctypes.data_as(up), fkeep.ctypes.data_as(up), best.ctypes.data_as(capi.c_double_p)))
    # bit p % 64 of word p / 64 -> column p (the words are little-endian: byte p / 8, bit p % 8)
    bits = lambda m: np.unpackbits(m.astype("<u8").view(np.uint8).reshape(len(m), 8 * W), axis=1, bitorder="little")[:, :K].astype(bool)
    return dict(arc_keep=bits(akeep), state_keep=bits(skeep), final_keep=bits(fkeep), best_final_cost=best,
                state_offsets=soff.astype(np.int64), arc_offsets=lat_arc_off, arc_keep_words=akeep, state_keep_words=skeep,
                final_keep_words=fkeep)


def _apply_score_point(g, a, label, scale, penalty):
    """ScaleTupleWeight (fstext/lattice-weight.h:233-241) then, with a label array, the penalty on arcs with a word
    (lat/lattice-functions.cc:1140-1143) on float32 arrays: what csrc/kh_latprune.hip applies to a weight."""
    s = np.asarray(scale, np.float64).reshape(4)
    zero = g == np.float32(np.inf)
    g64, a64 = np.where(zero, 0.0, g.astype(np.float64)), np.where(zero, 0.0, a.astype(np.float64))
    inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        g2 = np.where(zero, inf, (s[0] * g64 + s[1] * a64).astype(np.float32)).astype(np.float32)
        a2 = np.where(zero, inf, (s[2] * g64 + s[3] * a64).astype(np.float32)).astype(np.float32)
        if label is not None:
            g2 = np.where(label != 0, g2 + np.float32(penalty), g2).astype(np.float32)
    return g2, a2


def _empty_pruned():
    z, f = np.zeros(0, np.int32), np.zeros(0, np.float32)
    return dict(n_states=0, start=-1, arc_src=z, arc_dst=z, arc_label=z, arc_g=f, arc_a=f, arc_string=[], final_g=f, final_a=f,
                final_string=[], complete=True, kept_states=np.zeros(0, np.int64), kept_arcs=np.zeros(0, np.int64),
                final_kept=np.zeros(0, bool), ok=False)


def compact_lattice_prune(clats, points, beams, workspace_limit=None):
    """lattice-scale | lattice-add-penalty | lattice-prune --beam=B (PruneLattice, lat/lattice-functions.cc:186-265) for a
    batch of CompactLattices (dict layout of kaldi_io.read_compact_lattice) and a list of score points (score_point) in ONE
    device call; beams = one float or one per point.  Returns per lattice a list over the points of a CompactLattice dict in
    the same layout: the surviving states renumbered densely in the top-sorted order (what DeleteStates leaves; the start
    state becomes the first survivor), the surviving arcs in their order within a state, the weights those AFTER the point
    (what the pipe carries into lattice-prune), the strings untouched.  Each dict also carries kept_states, kept_arcs
    (indices into the input dict, in the output's order), final_kept (per surviving state) and ok; ok is False when nothing
    survives - PruneLattice returns false - and the dict then has n_states = 0 and start = -1.  A lattice without states or
    without a start state gives that for every point, without a device call."""
    K = len(points)
    has_start = [int(c["n_states"]) > 0 and int(c.get("start", 0)) >= 0 for c in clats]    # :203
    csrs = [compact_lattice_to_prune_csr(c) for c, ok in zip(clats, has_start) if ok]
    if not csrs:
        return [[_empty_pruned() for _ in range(K)] for _ in clats]
    raw = compact_lattice_prune_raw(csrs, [L["start"] for L in csrs], points, beams, workspace_limit)
    soff, aoff = raw["state_offsets"], raw["arc_offsets"]
    inf, empty = np.float32(np.inf), np.zeros(0, np.int32)
    out = []
    i = -1
    for c, ok in zip(clats, has_start):
        if not ok:
            out.append([_empty_pruned() for _ in range(K)])
            continue
        i += 1
        L = csrs[i]
        n = L["n_states"]
        ak, sk, fk = (raw["arc_keep"][aoff[i]:aoff[i + 1]], raw["state_keep"][soff[i]:soff[i + 1]],
                      raw["final_keep"][soff[i]:soff[i + 1]])
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(L["arc_offsets"]))
        dst = L["arc_nextstate"].astype(np.int64)
        astr = np.empty(len(src), object)
        for j, x in enumerate(c["arc_string"]):
            astr[j] = x
        fstr = np.empty(n, object)
        for s, x in enumerate(c["final_string"]):
            fstr[s] = x
        row = []
        for p, (scale, pen) in enumerate(points):
            ks = np.flatnonzero(sk[:, p])
            if len(ks) == 0:
                row.append(_empty_pruned())
                continue
            ka = np.flatnonzero(ak[:, p])
            new = np.cumsum(sk[:, p]) - 1
            g, a = _apply_score_point(L["arc_graph"][ka], L["arc_acoustic"][ka], L["arc_label"][ka], scale, pen)
            fg, fa = _apply_score_point(L["final_graph"][ks], L["final_acoustic"][ks], None, scale, pen)
            kept = fk[ks, p]
            kept_states, kept_arcs = L["state_of"][ks], L["perm"][ka]
            row.append(dict(n_states=len(ks), start=int(new[L["start"]]), arc_src=new[src[ka]].astype(np.int32),
                            arc_dst=new[dst[ka]].astype(np.int32), arc_label=L["arc_label"][ka], arc_g=g, arc_a=a,
                            arc_string=astr[kept_arcs].tolist(), final_g=np.where(kept, fg, inf).astype(np.float32),
                            final_a=np.where(kept, fa, inf).astype(np.float32),
                            final_string=[x if k else empty for x, k in zip(fstr[kept_states].tolist(), kept.tolist())],
                            complete=True, kept_states=kept_states, kept_arcs=kept_arcs, final_kept=kept, ok=True))
        out.append(row)
    return out


def compact_lattice_prune_last_timings():
    """Milliseconds the last compact_lattice_prune call of this thread spent in host preparation / upload / kernels /
    download (the allocations are in none of the four), in the whole C call, and the number of launches of the sweep kernel."""
    return _timings(lib().kh_compact_lattice_prune_last_timings, _MS5, ("launches",))


# ---------------------------------------------------------------- oracle path and depth (csrc/kh_latoracle.hip)
def _mask_words(m, K):
    """bool [n x K] -> the uint64 words of kh_compact_lattice_prune's masks [n x ceil(K / 64)]."""
    m = np.asarray(m, bool).reshape(-1, K)
    W = (K + 63) // 64
    b = np.zeros((len(m), 8 * W), np.uint8)
    packed = np.packbits(m, axis=1, bitorder="little")
    b[:, :packed.shape[1]] = packed
    return np.ascontiguousarray(b.view("<u8").astype(np.uint64).reshape(len(m), W))


def _csr_is_final(L):
    if "is_final" in L:
        return np.asarray(L["is_final"], bool)
    fg, fa = np.asarray(L["final_graph"], np.float32), np.asarray(L["final_acoustic"], np.float32)
    return ~((fg == np.inf) & (fa == np.inf))          # Final(s) != Weight::Zero()


def compact_lattice_oracle_raw(csrs, starts, refs, wildcards, masks=None, workspace_limit=None):
    """kh_compact_lattice_oracle on CSR dicts (compact_lattice_to_prune_csr's layout, top-sorted), starts = the start state
    of each, refs = one integer sequence per lattice, wildcards = labels that count as epsilon.  masks: None (one point,
    everything kept) or dict(arc_keep, state_keep, final_keep = bool [arcs or states of the whole batch x n_points]) as
    compact_lattice_prune_raw returns; where the dict also carries its arc_keep_words, state_keep_words, final_keep_words
    those go to the device as they are and the bool arrays are not packed again.  When every dict carries arc_frames and final_frames (the lengths of the
    transition-id strings) the frame sums are returned too.  Returns dict(errors [n_lats x n_points], counts
    [n_lats x n_points x 4: correct, sub, ins, del], path_len, paths [list of lists of int32 arrays: CSR arc numbers
    within the lattice], final_state, frame_sum [int64, or None])."""
    n = len(csrs)
    if n == 0 or len(refs) != n:
        raise KhError("compact_lattice_oracle: no lattices, or not one reference per lattice")
    K = 1 if masks is None else int(np.asarray(masks["final_keep"]).shape[1])
    soff, aoff, _, cat = _batch_csr(csrs)
    lab, ns = cat("arc_label", np.int32), cat("arc_nextstate", np.int32)
    fin = np.ascontiguousarray(np.concatenate([_csr_is_final(L) for L in csrs]).astype(np.int32))
    st = np.ascontiguousarray(np.asarray(starts, np.int32).reshape(n))
    roff = np.zeros(n + 1, np.int64)
    roff[1:] = np.cumsum([len(r) for r in refs])
    rw = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int32).reshape(-1) for r in refs] + [np.zeros(0, np.int32)]))
    wild = np.ascontiguousarray(np.unique(np.asarray(list(wildcards), np.int32)))
    frames = all("arc_frames" in L and "final_frames" in L for L in csrs)
    af, ff = (cat("arc_frames", np.int32), cat("final_frames", np.int32)) if frames else (None, None)
    ip, up, lp = capi.c_int32_p, capi.c_uint64_p, capi.c_int64_p
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    ak = sk = fk = None
    if masks is not None:
        W = (K + 63) // 64
        words = lambda k, rows: (np.ascontiguousarray(np.asarray(masks[k + "_words"], np.uint64).reshape(rows, W))
                                 if k + "_words" in masks else _mask_words(masks[k], K))
        ak, sk, fk = words("arc_keep", len(lab)), words("state_keep", int(soff[-1])), words("final_keep", int(soff[-1]))
        if not (len(ak) == len(lab) and len(sk) == len(fk) == int(soff[-1])):
            raise KhError("compact_lattice_oracle: the masks have %d, %d, %d rows for %d arcs and %d states"
                          % (len(ak), len(sk), len(fk), len(lab), int(soff[-1])))
    poff = _path_room(soff, K)
    err, cnt = np.empty(n * K, np.int32), np.empty(n * K * 4, np.int32)
    plen, pfin = np.empty(n * K, np.int32), np.empty(n * K, np.int32)
    parcs = np.empty(int(poff[-1]), np.int32)
    fsum = np.zeros(n * K, np.int64)
    with _workspace_limit(lib().kh_compact_lattice_oracle_set_workspace_limit, workspace_limit):
        check(lib().kh_compact_lattice_oracle(
            n, ptr(soff, ip), ptr(st, ip), ptr(aoff, lp), ptr(lab, ip), ptr(ns, ip), ptr(fin, ip), ptr(roff, lp), ptr(rw, ip),
            len(wild), ptr(wild, ip), K, ptr(ak, up), ptr(sk, up), ptr(fk, up), ptr(af, ip), ptr(ff, ip), ptr(err, ip),
            ptr(cnt, ip), ptr(plen, ip), ptr(parcs, ip), ptr(poff, lp), ptr(pfin, ip), ptr(fsum, lp) if frames else None))
    return dict(errors=err.reshape(n, K), counts=cnt.reshape(n, K, 4), path_len=plen.reshape(n, K),
                paths=_split_paths(parcs, poff, plen, n, K),
                final_state=pfin.reshape(n, K), frame_sum=fsum.reshape(n, K) if frames else None)


def _prune_csr_state_times(L):
    """CompactLatticeStateTimes (lat/lattice-functions.cc:69-106) on a CSR dict with arc_frames, counted from its start
    state: times [-1 = not reachable].  Raises where the reference's assertion :87 fails."""
    n, start = int(L["n_states"]), int(L["start"])
    off, nxt, af = np.asarray(L["arc_offsets"], np.int64), np.asarray(L["arc_nextstate"], np.int64), np.asarray(L["arc_frames"], np.int64)
    times = np.full(n, -1, np.int64)
    times[start] = 0
    for s in range(start, n):
        if times[s] < 0 or off[s] == off[s + 1]:
            continue
        d, t = nxt[off[s]:off[s + 1]], times[s] + af[off[s]:off[s + 1]]
        unset = times[d] < 0
        times[d[unset]] = t[unset]
        if not np.array_equal(times[d], t):
            raise KhError("KALDI_ASSERT: at CompactLatticeStateTimes:lattice-functions.cc:87, failed: "
                          "(*times)[arc.nextstate] == cur_time + arc_len")
    return times


def _oracle_csr(clat):
    """compact_lattice_to_prune_csr plus is_final and, when the dict carries the strings, arc_frames / final_frames."""
    L = compact_lattice_to_prune_csr(clat)
    L["is_final"] = _csr_is_final(L)
    if "arc_string" in clat and "final_string" in clat:
        L["arc_frames"] = np.asarray([len(clat["arc_string"][j]) for j in L["perm"]], np.int32).reshape(-1)
        L["final_frames"] = np.asarray([len(clat["final_string"][s]) for s in L["state_of"]], np.int32).reshape(-1)
    return L


def compact_lattice_depth(clat):
    """CompactLatticeDepth (lat/lattice-functions.cc:574-602) after TopSortCompactLatticeIfNeeded (latbin/lattice-depth.cc:65):
    (depth [float32], t) with t from CompactLatticeStateTimes (:69-106).  Depth is 1.0 and t = 0 when there is no start
    state (:581-584) or no final state is reachable (where the reference divides by zero)."""
    if int(clat["n_states"]) == 0 or int(clat.get("start", 0)) < 0:
        return np.float32(1.0), 0
    L = _oracle_csr(clat)
    times = _prune_csr_state_times(L)
    ends = times + L["final_frames"]
    ok = L["is_final"] & (times >= 0)
    t = int(ends[ok].max()) if ok.any() else 0
    if t == 0:
        return np.float32(1.0), 0
    num_arc_frames = int(L["arc_frames"].sum(dtype=np.int64)) + int(L["final_frames"].sum(dtype=np.int64))
    return np.float32(num_arc_frames) / np.float32(t), t


def compact_lattice_oracle(clats, refs, wildcards=(), points=None, beams=None, workspace_limit=None):
    """lattice-oracle (latbin/lattice-oracle.cc:313-421) and lattice-depth for a batch of CompactLattices (dict layout of
    kaldi_io.read_compact_lattice; without the strings there is no depth) and one reference word sequence each.  With beams
    (one per point; points = one score_point or one per beam, default the identity) every lattice is first pruned on the
    device at each beam - `lattice-scale | lattice-prune --beam=b` - and the masks go straight into the oracle call.
    Returns per lattice a list over the points of dict(errors [-1: no path, the reference's "Best-path failed"], correct,
    sub, ins, del, words = the oracle word sequence, path_arcs = the path as indices into the dict's arc arrays, depth,
    num_frames = CompactLatticeDepth of what the point keeps [None without strings]).  errors and
    correct + sub + del = the reference's length are the reference binary's; which of several equal-cost paths is reported
    follows the rule in include/kaldi_hip.h, not OpenFst's ShortestPath."""
    if beams is None:
        K = 1
    else:
        bm = np.asarray(beams, np.float32).reshape(-1)
        K = len(bm)
        points = [score_point()] if points is None else list(points)
        if len(points) == 1:
            points = points * K
        if len(points) != K:
            raise KhError("compact_lattice_oracle: %d score points for %d beams" % (len(points), K))
    wild = set(int(w) for w in wildcards)
    none = lambda: dict(errors=-1, correct=0, sub=0, ins=0, words=np.zeros(0, np.int32), path_arcs=np.zeros(0, np.int64),
                        depth=np.float32(1.0), num_frames=0, **{"del": 0})
    has_start = [int(c["n_states"]) > 0 and int(c.get("start", 0)) >= 0 for c in clats]
    csrs = [_oracle_csr(c) for c, ok in zip(clats, has_start) if ok]
    if not csrs:
        return [[none() for _ in range(K)] for _ in clats]
    starts = [L["start"] for L in csrs]
    masks = None if beams is None else compact_lattice_prune_raw(csrs, starts, points, bm, workspace_limit)
    raw = compact_lattice_oracle_raw(csrs, starts, [r for r, ok in zip(refs, has_start) if ok], wild, masks, workspace_limit)
    out = []
    i, s0 = -1, 0
    for c, ok in zip(clats, has_start):
        if not ok:
            out.append([none() for _ in range(K)])
            continue
        i += 1
        L = csrs[i]
        n = int(L["n_states"])
        labels = np.asarray(L["arc_label"], np.int32)
        eps = (labels == 0) | np.isin(labels, list(wild))
        ends = None
        if raw["frame_sum"] is not None:
            times = _prune_csr_state_times(L)
            ends = np.where(L["is_final"] & (times >= 0), times + L["final_frames"], 0)
        row = []
        for p in range(K):
            r = none()
            if ends is not None:
                live = ends if masks is None else np.where(masks["state_keep"][s0:s0 + n, p] & masks["final_keep"][s0:s0 + n, p], ends, 0)
                t = int(live.max())
                if t > 0:
                    r["depth"], r["num_frames"] = np.float32(int(raw["frame_sum"][i, p])) / np.float32(t), t
            else:
                r["depth"] = r["num_frames"] = None
            if raw["errors"][i, p] >= 0:
                arcs = raw["paths"][i][p]
                cnt = raw["counts"][i, p]
                r.update(errors=int(raw["errors"][i, p]), correct=int(cnt[0]), sub=int(cnt[1]), ins=int(cnt[2]),
                         words=labels[arcs][~eps[arcs]], path_arcs=L["perm"][arcs].astype(np.int64))
                r["del"] = int(cnt[3])
            row.append(r)
        out.append(row)
        s0 += n
    return out


def compact_lattice_oracle_last_timings():
    """Milliseconds the last compact_lattice_oracle call of this thread spent in host preparation / upload / kernel /
    download (the allocations are in none of the four), in the whole C call, and the number of kernel launches."""
    return _timings(lib().kh_compact_lattice_oracle_last_timings, _MS5, ("launches",))


# ---------------------------------------------------------------- minimum Bayes risk decoding (csrc/kh_latmbr.hip)
def compact_lattice_mbr_prepare(clat):
    """PrepareLatticeAndInitStats (lat/sausages.cc:268-315) on a CompactLattice dict (layout of
    kaldi_io.read_compact_lattice, with the strings): CreateSuperFinal by its own rule
    (fstext/pre-determinize-inl.h:693-730: a single final state with weight One and no arcs is left alone; otherwise a new
    last state becomes the only final state, and every old final state gets, in ascending state order, an epsilon arc to it
    that carries its final weight, appended behind its other arcs); then the states are renumbered by
    compact_lattice_top_order, only if the result is not sorted as it stands; then CompactLatticeStateTimes.  Returns the
    CSR dict of compact_lattice_to_csr plus start = 0, arc_frames, state_times (int32; -1 = not reachable), and
    n_input_arcs (CSR arcs whose perm is >= that are the added ones).  Raises where the reference would fail (a cycle,
    inconsistent times) and where the last state does not come out as the single final state - the reference assumes it
    (:323-327), which holds for a lattice without dead ends."""
    n = int(clat["n_states"])
    fg, fa = np.asarray(clat["final_g"], np.float32), np.asarray(clat["final_a"], np.float32)
    src, dst = np.asarray(clat["arc_src"], np.int64), np.asarray(clat["arc_dst"], np.int64)
    finals = np.flatnonzero(~((fg == np.inf) & (fa == np.inf)))                          # :701-706
    n_in = len(src)
    aug = dict(clat)
    single = len(finals) == 1 and fg[finals[0]] == 0 and fa[finals[0]] == 0 and len(clat["final_string"][finals[0]]) == 0 \
        and not np.any(src == finals[0])                                                # :707-714
    if not single:
        empty = np.zeros(0, np.int32)
        k = len(finals)
        new_fg, new_fa = np.full(n + 1, np.inf, np.float32), np.full(n + 1, np.inf, np.float32)
        new_fg[n] = new_fa[n] = 0.0                                                      # :716-717
        fstr = [empty for _ in range(n + 1)]
        aug.update(n_states=n + 1, arc_src=np.concatenate([src, finals]).astype(np.int32),          # :718-728
                   arc_dst=np.concatenate([dst, np.full(k, n, np.int64)]).astype(np.int32),
                   arc_label=np.concatenate([np.asarray(clat["arc_label"], np.int32), np.zeros(k, np.int32)]),
                   arc_g=np.concatenate([np.asarray(clat["arc_g"], np.float32), fg[finals]]),
                   arc_a=np.concatenate([np.asarray(clat["arc_a"], np.float32), fa[finals]]),
                   arc_string=list(clat["arc_string"]) + [np.asarray(clat["final_string"][s], np.int32) for s in finals],
                   final_g=new_fg, final_a=new_fa, final_string=fstr)
    if int(aug["n_states"]) == 0 or int(aug.get("start", 0)) < 0:
        raise KhError("compact_lattice_mbr_prepare: the lattice has no start state")
    L = compact_lattice_to_csr(aug)                                                      # :276-280
    L["start"] = 0
    L["arc_frames"] = np.asarray([len(aug["arc_string"][j]) for j in L["perm"]], np.int32).reshape(-1)
    L["state_times"] = _prune_csr_state_times(L).astype(np.int32)                        # :281
    L["n_input_arcs"] = n_in
    N = int(L["n_states"])
    is_final = _csr_is_final(L)
    if not (is_final[N - 1] and is_final.sum() == 1 and L["arc_offsets"][N - 1] == L["arc_offsets"][N]):
        raise KhError("compact_lattice_mbr_prepare: after the topological sort the final state is state %s of %d, not the "
                      "last one (the lattice has dead ends; the reference assumes it has none, lat/sausages.cc:323-327)"
                      % (np.flatnonzero(is_final).tolist(), N))
    return L


def compact_lattice_mbr_raw(csrs, points, hyps, do_mbr=True, workspace_limit=None):
    """kh_compact_lattice_mbr on prepared CSR dicts (compact_lattice_mbr_prepare), points as compact_lattice_best_paths_raw
    takes them, hyps[i][p] = the initial word sequence of lattice i at point p.  Returns a list per lattice of a list per
    point of dict(words [int32], bayes_risk [float64, L_], iterations, sausage_stats [list over the bins of lists of
    (word, float32)], sausage_times, one_best_times [float32 n x 2], one_best_confidences [float32]).  The room for the
    ragged outputs is a guess from the hypotheses; when a pair does not fit, the call is made once more with the room the
    first one reported."""
    n, K = len(csrs), len(points)
    if n == 0 or K == 0:
        raise KhError("compact_lattice_mbr: no lattices or no score points")
    soff, aoff, _, cat = _batch_csr(csrs)
    lab, ns = cat("arc_label", np.int32), cat("arc_nextstate", np.int32)
    g, a = cat("arc_graph", np.float32), cat("arc_acoustic", np.float32)
    fg, fa = cat("final_graph", np.float32), cat("final_acoustic", np.float32)
    times = cat("state_times", np.int32)
    st = np.ascontiguousarray(np.asarray([int(L.get("start", 0)) for L in csrs], np.int32))
    scales, pens = _point_arrays(points)
    flat = [np.asarray(hyps[i][p], np.int32).reshape(-1) for i in range(n) for p in range(K)]
    hoff = np.zeros(n * K + 1, np.int64)
    hoff[1:] = np.cumsum([len(h) for h in flat])
    hw = np.ascontiguousarray(np.concatenate(flat + [np.zeros(0, np.int32)]))
    n_labels = np.repeat([len(np.unique(L["arc_label"])) + 1 for L in csrs], K)
    nw, nb, nst = np.zeros(n * K, np.int32), np.zeros(n * K, np.int32), np.zeros(n * K, np.int32)
    risk, iters = np.zeros(n * K, np.float64), np.zeros(n * K, np.int32)
    room_w = np.diff(hoff) + 8
    room_b = 2 * room_w + 1
    room_s = room_b * np.minimum(n_labels, 32)
    ip, fp, lp, dp = capi.c_int32_p, capi.c_float_p, capi.c_int64_p, capi.c_double_p
    ptr = lambda x, t: x.ctypes.data_as(t)
    offs = lambda room: np.ascontiguousarray(np.concatenate([[0], np.cumsum(room)]).astype(np.int64))
    with _workspace_limit(lib().kh_compact_lattice_mbr_set_workspace_limit, workspace_limit):
        for attempt in range(2):
            woff, boff, soff2 = offs(room_w), offs(room_b), offs(room_s)
            words, obt, obc = np.zeros(int(woff[-1]), np.int32), np.zeros(2 * int(woff[-1]), np.float32), np.zeros(int(woff[-1]), np.float32)
            bsz, bt = np.zeros(int(boff[-1]), np.int32), np.zeros(2 * int(boff[-1]), np.float32)
            sw, sp = np.zeros(int(soff2[-1]), np.int32), np.zeros(int(soff2[-1]), np.float32)
            rc = lib().kh_compact_lattice_mbr(
                n, ptr(soff, ip), ptr(st, ip), ptr(aoff, lp), ptr(lab, ip), ptr(ns, ip), ptr(g, fp), ptr(a, fp), ptr(fg, fp),
                ptr(fa, fp), ptr(times, ip), K, ptr(scales, dp), ptr(pens, fp), ptr(hoff, lp), ptr(hw, ip), 1 if do_mbr else 0,
                ptr(nw, ip), ptr(woff, lp), ptr(words, ip), ptr(obt, fp), ptr(obc, fp), ptr(risk, dp), ptr(iters, ip),
                ptr(nb, ip), ptr(boff, lp), ptr(bsz, ip), ptr(bt, fp), ptr(nst, ip), ptr(soff2, lp), ptr(sw, ip), ptr(sp, fp))
            if rc != 0 and attempt == 0 and b"do not fit the room" in lib().kh_last_error():
                room_w, room_b, room_s = nw.astype(np.int64), nb.astype(np.int64), nst.astype(np.int64)
                continue
            check(rc)
            break
    out = []
    for i in range(n):
        row = []
        for p in range(K):
            o = i * K + p
            w0, b0, s0 = int(woff[o]), int(boff[o]), int(soff2[o])
            sizes = bsz[b0:b0 + nb[o]]
            ends = s0 + np.cumsum(sizes)
            stats = [list(zip(sw[e - k:e].tolist(), sp[e - k:e])) for k, e in zip(sizes.tolist(), ends.tolist())]
            row.append(dict(words=words[w0:w0 + nw[o]].copy(), bayes_risk=float(risk[o]), iterations=int(iters[o]),
                            sausage_stats=stats, sausage_times=bt[2 * b0:2 * (b0 + nb[o])].reshape(-1, 2).copy(),
                            one_best_times=obt[2 * w0:2 * (w0 + nw[o])].reshape(-1, 2).copy(),
                            one_best_confidences=obc[w0:w0 + nw[o]].copy()))
        out.append(row)
    return out


def compact_lattice_mbr(clats, points=None, one_bests=None, do_mbr=True, workspace_limit=None):
    """MinimumBayesRisk (lat/sausages.{h,cc}: lattice-mbr-decode, lattice-to-ctm-conf) for a batch of CompactLattices (dict
    layout of kaldi_io.read_compact_lattice, with the strings) and a list of score points (score_point; None = the lattice
    as it is) in ONE call.  one_bests: None, or per lattice a word sequence that is the initial hypothesis at every point
    (the class's second constructor; lattice-to-ctm-conf's three-argument form passes do_mbr=False with it).  Without it the
    initial hypothesis is the word sequence of compact_lattice_best_paths on the prepared lattice at the same points.  The
    reference takes fst::ShortestPath there (:329-345); both find a path of the smallest cost, but where best paths tie in
    cost they may return different ones, and the initial hypothesis - and with do_mbr=False the result - may then differ.
    Returns per lattice a list over the points of dict(words [int32, GetOneBest], bayes_risk [float32, GetBayesRisk],
    sausage_stats [per bin a list of (word, float32), most likely first], sausage_times, one_best_times [float32 n x 2],
    one_best_confidences [float32], iterations); None for every point of a lattice without states or start state."""
    points = [score_point()] if points is None else list(points)
    K = len(points)
    has_start = [int(c["n_states"]) > 0 and int(c.get("start", 0)) >= 0 for c in clats]
    csrs = [compact_lattice_mbr_prepare(c) for c, ok in zip(clats, has_start) if ok]
    if not csrs:
        return [[None] * K for _ in clats]
    if one_bests is None:
        plen, paths, _, _, _ = compact_lattice_best_paths_raw(csrs, points, workspace_limit)
        hyps = []
        for i, L in enumerate(csrs):
            if np.any(plen[i] < 0):
                raise KhError("compact_lattice_mbr: lattice %d has no path to its final state" % i)
            labels = np.asarray(L["arc_label"], np.int32)
            hyps.append([labels[paths[i][p]][labels[paths[i][p]] != 0] for p in range(K)])
    else:
        kept = [np.asarray(w, np.int32).reshape(-1) for w, ok in zip(one_bests, has_start) if ok]
        hyps = [[w] * K for w in kept]
    raw = compact_lattice_mbr_raw(csrs, points, hyps, do_mbr, workspace_limit)
    for row in raw:
        for r in row:
            r["bayes_risk"] = np.float32(r["bayes_risk"])
    it = iter(raw)
    return [next(it) if ok else [None] * K for ok in has_start]


def compact_lattice_mbr_last_timings():
    """Milliseconds the last compact_lattice_mbr_raw call of this thread spent in host preparation (alpha and the arc
    posteriors among it) / uploads / kernels / downloads, in the whole C call, in the host's part of MbrDecode, and the
    number of kernel launches, rounds of the host loop, and AccStats() calls summed over the (lattice, point) pairs."""
    return _timings(lib().kh_compact_lattice_mbr_last_timings, _MS5 + ("host_loop_ms",), ("launches", "rounds", "acc_stats"))


ALIGN_OK, ALIGN_ERROR, ALIGN_EMPTY, ALIGN_TOO_MANY_STATES, ALIGN_FATAL = range(5)


def compact_lattice_align_csr(clat):
    """CompactLattice dict (kaldi_io.read_compact_lattice, with the strings) -> the top-sorted CSR dict of
    compact_lattice_to_csr plus start, arc_string and final_string (lists of int32 arrays in CSR order)."""
    n = int(clat["n_states"])
    start = int(clat.get("start", 0))
    if n == 0 or start < 0:
        return dict(n_states=0, start=-1, arc_offsets=np.zeros(1, np.int64), arc_label=np.zeros(0, np.int32),
                    arc_nextstate=np.zeros(0, np.int32), arc_graph=np.zeros(0, np.float32), arc_acoustic=np.zeros(0, np.float32),
                    final_graph=np.zeros(0, np.float32), final_acoustic=np.zeros(0, np.float32), arc_string=[], final_string=[])
    order = compact_lattice_top_order(clat)
    L = compact_lattice_to_csr(clat)
    L["start"] = start if order is None else int(order[start])
    L["arc_string"] = [np.asarray(clat["arc_string"][j], np.int32).reshape(-1) for j in L["perm"]]
    L["final_string"] = [np.asarray(clat["final_string"][s], np.int32).reshape(-1) for s in L["state_of"]]
    return L


def compact_lattice_align_words_pack(csrs, tmodel, wbinfo, max_states=0):
    """The arguments of kh_compact_lattice_align_words as contiguous arrays: a dict in the C call's order of names."""
    n = len(csrs)
    soff, aoff, _, cat = _batch_csr(csrs)
    arc_strings = [x for L in csrs for x in L["arc_string"]]
    final_strings = [x for L in csrs for x in L["final_string"]]
    offs = lambda strs: np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(x) for x in strs])]).astype(np.int64))
    flat = lambda strs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in strs] + [np.zeros(0, np.int32)]))
    i32 = lambda x: np.ascontiguousarray(np.asarray(x).astype(np.int32).reshape(-1))
    ms = np.broadcast_to(np.asarray(max_states, np.int64), (n,)) if np.ndim(max_states) == 0 else np.asarray(max_states, np.int64)
    if np.any(ms < 0) or np.any(ms >= 2 ** 31):
        raise KhError("compact_lattice_align_words: max_states out of range")
    return dict(lat_state_offsets=soff, lat_start=i32([int(L.get("start", 0)) for L in csrs]),
                arc_offsets=aoff, arc_label=cat("arc_label", np.int32),
                arc_nextstate=cat("arc_nextstate", np.int32), arc_graph=cat("arc_graph", np.float32),
                arc_acoustic=cat("arc_acoustic", np.float32), arc_string_offsets=offs(arc_strings), arc_strings=flat(arc_strings),
                final_graph=cat("final_graph", np.float32), final_acoustic=cat("final_acoustic", np.float32),
                final_string_offsets=offs(final_strings), final_strings=flat(final_strings),
                tid_phone=i32(tmodel["tid2phone"]), tid_is_final=i32(tmodel["tid_is_final"]),
                tid_is_self_loop=i32(tmodel["tid_is_self_loop"]), phone_type=i32(wbinfo["phone_to_type"]),
                reorder=int(bool(wbinfo["reorder"])), silence_label=int(wbinfo["silence_label"]),
                partial_word_label=int(wbinfo["partial_word_label"]), max_states=i32(ms))


def compact_lattice_align_words_call(A, room_s, room_a, room_w, fill=0):
    """One kh_compact_lattice_align_words call on compact_lattice_align_words_pack's arrays with the given room per lattice
    (states, arcs, transition-ids).  Returns (rc, counts, outputs): counts = dict(status, n_states, n_arcs, n_tuples,
    n_string_words), outputs = dict of the offset arrays and the output arrays, created filled with `fill`."""
    n = len(A["lat_start"])
    status, ns, na, nt = (np.zeros(n, np.int32) for _ in range(4))
    nw = np.zeros(n, np.int64)
    offs = lambda r: np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.asarray(r, np.int64).reshape(n))]).astype(np.int64))
    so, ao, wo = offs(room_s), offs(room_a), offs(room_w)
    f32 = lambda k: np.full(int(k), fill, np.float32)
    i32 = lambda k: np.full(int(k), fill, np.int32)
    O = dict(state_offsets=so, arc_offsets=ao, string_offsets=wo, final_graph=f32(so[-1]), final_acoustic=f32(so[-1]),
             arc_src=i32(ao[-1]), arc_nextstate=i32(ao[-1]), arc_label=i32(ao[-1]), arc_graph=f32(ao[-1]), arc_acoustic=f32(ao[-1]),
             arc_string_len=i32(ao[-1]), strings=i32(wo[-1]))
    ip, fp, lp = capi.c_int32_p, capi.c_float_p, capi.c_int64_p
    ptr = lambda x, t: x.ctypes.data_as(t)
    rc = lib().kh_compact_lattice_align_words(
        n, ptr(A["lat_state_offsets"], ip), ptr(A["lat_start"], ip), ptr(A["arc_offsets"], lp), ptr(A["arc_label"], ip),
        ptr(A["arc_nextstate"], ip), ptr(A["arc_graph"], fp), ptr(A["arc_acoustic"], fp), ptr(A["arc_string_offsets"], lp),
        ptr(A["arc_strings"], ip), ptr(A["final_graph"], fp), ptr(A["final_acoustic"], fp), ptr(A["final_string_offsets"], lp),
        ptr(A["final_strings"], ip), len(A["tid_phone"]) - 1, ptr(A["tid_phone"], ip), ptr(A["tid_is_final"], ip),
        ptr(A["tid_is_self_loop"], ip), len(A["phone_type"]), ptr(A["phone_type"], ip), A["reorder"], A["silence_label"],
        A["partial_word_label"], ptr(A["max_states"], ip), ptr(status, ip), ptr(ns, ip), ptr(na, ip), ptr(nt, ip), ptr(nw, lp),
        ptr(so, lp), ptr(ao, lp), ptr(wo, lp), ptr(O["final_graph"], fp), ptr(O["final_acoustic"], fp), ptr(O["arc_src"], ip),
        ptr(O["arc_nextstate"], ip), ptr(O["arc_label"], ip), ptr(O["arc_graph"], fp), ptr(O["arc_acoustic"], fp),
        ptr(O["arc_string_len"], ip), ptr(O["strings"], ip))
    return rc, dict(status=status, n_states=ns, n_arcs=na, n_tuples=nt, n_string_words=nw), O


def compact_lattice_align_words_raw(csrs, tmodel, wbinfo, max_states=0, workspace_limit=None, room=None):
    """kh_compact_lattice_align_words on CSR dicts (compact_lattice_align_csr).  Returns per lattice dict(status, n_tuples,
    n_states, final [n x 2 float32], arcs [(src, dst, label, g, a, string)]).  room: None = a guess from the input, run once
    more with the room the first call's counts name when they exceed it; or (states, arcs, transition-ids) per lattice, taken
    as it is."""
    n = len(csrs)
    if n == 0:
        raise KhError("compact_lattice_align_words: no lattices")
    A = compact_lattice_align_words_pack(csrs, tmodel, wbinfo, max_states)
    if len(A["tid_phone"]) != len(A["tid_is_final"]) or len(A["tid_phone"]) != len(A["tid_is_self_loop"]) or len(A["tid_phone"]) < 2:
        raise KhError("compact_lattice_align_words: the three transition-id tables differ in length")
    if room is None:
        words = np.asarray([sum(len(x) for x in L["arc_string"]) + sum(len(x) for x in L["final_string"]) for L in csrs], np.int64)
        arcs = np.diff(A["lat_state_offsets"]).astype(np.int64) + np.asarray([int(L["arc_offsets"][-1]) for L in csrs], np.int64)
        rooms = [2 * arcs + 4, 2 * arcs + 4, 2 * words + 4]
    else:
        rooms = [np.asarray(r, np.int64).reshape(n) for r in room]
    with _workspace_limit(lib().kh_compact_lattice_align_words_set_workspace_limit, workspace_limit):
        rc, cnt, O = compact_lattice_align_words_call(A, *rooms)
        need = [cnt["n_states"].astype(np.int64), cnt["n_arcs"].astype(np.int64), cnt["n_string_words"].astype(np.int64)]
        if rc != 0 and room is None and any(np.any(x > r) for x, r in zip(need, rooms)):   # the counts are always written
            rc, cnt, O = compact_lattice_align_words_call(A, *need)
        check(rc)
    so, ao, wo, alen, strs = O["state_offsets"], O["arc_offsets"], O["string_offsets"], O["arc_string_len"], O["strings"]
    out = []
    for i in range(n):
        s0, a0, w0, ns, na = int(so[i]), int(ao[i]), int(wo[i]), int(cnt["n_states"][i]), int(cnt["n_arcs"][i])
        ends = w0 + np.cumsum(alen[a0:a0 + na])
        arcs = [(int(O["arc_src"][a0 + k]), int(O["arc_nextstate"][a0 + k]), int(O["arc_label"][a0 + k]), O["arc_graph"][a0 + k],
                 O["arc_acoustic"][a0 + k], tuple(strs[int(ends[k]) - int(alen[a0 + k]):int(ends[k])].tolist())) for k in range(na)]
        out.append(dict(status=int(cnt["status"][i]), n_tuples=int(cnt["n_tuples"][i]), n_states=ns,
                        final=np.stack([O["final_graph"][s0:s0 + ns], O["final_acoustic"][s0:s0 + ns]], axis=1), arcs=arcs))
    return out


def compact_lattice_align_words(clats, tmodel, wbinfo, max_states=0, workspace_limit=None):
    """WordAlignLattice (lat/word-align-lattice.cc; lattice-align-words) for a batch of CompactLattices (dicts of
    kaldi_io.read_compact_lattice, with the strings) in ONE call.  tmodel: kaldi_io.read_transition_model's dict (tid2phone,
    tid_is_final, tid_is_self_loop); wbinfo: kaldi_io.read_word_boundary_info's; max_states: one number or one per lattice
    (0 = no limit).  Returns per lattice dict(status [ALIGN_*], n_tuples, clat): clat the aligned lattice in the same dict
    layout, numbered by the rule of include/kaldi_hip.h (top-sorted, start state 0), or None where there is none (empty
    input, too many states, fatal, or no path left).  A lattice that is not top-sorted is renumbered by
    compact_lattice_top_order first."""
    raw = compact_lattice_align_words_raw([compact_lattice_align_csr(c) for c in clats], tmodel, wbinfo, max_states, workspace_limit)
    out = []
    for r in raw:
        c = None
        if r["n_states"] > 0:
            arcs, m = r["arcs"], r["n_states"]
            c = dict(n_states=m, start=0, arc_src=np.asarray([x[0] for x in arcs], np.int32),
                     arc_dst=np.asarray([x[1] for x in arcs], np.int32), arc_label=np.asarray([x[2] for x in arcs], np.int32),
                     arc_g=np.asarray([x[3] for x in arcs], np.float32), arc_a=np.asarray([x[4] for x in arcs], np.float32),
                     arc_string=[np.asarray(x[5], np.int32) for x in arcs], final_g=r["final"][:, 0].copy(),
                     final_a=r["final"][:, 1].copy(), final_string=[np.zeros(0, np.int32) for _ in range(m)])
        out.append(dict(status=r["status"], n_tuples=r["n_tuples"], clat=c))
    return out


def compact_lattice_align_words_last_timings():
    """Milliseconds the last compact_lattice_align_words_raw call of this thread spent in host preparation / uploads / kernels
    / downloads, in the whole C call, in the host's sort and merge, and the number of kernel launches, of lattices run again
    with more room, and of tuples over all lattices."""
    return _timings(lib().kh_compact_lattice_align_words_last_timings, _MS5 + ("host_finish_ms",),
                    ("launches", "run_again", "tuples"))


RESCORE_OK, RESCORE_EMPTY, RESCORE_INCONSISTENT_TIMES, RESCORE_FEATURES_TOO_SHORT, RESCORE_BAD_TID, RESCORE_MISMATCH = range(6)
RESCORE_CYCLIC = 6      # compact_lattice_rescore's own: fst::TopSort failed ("Cycles detected in lattice."); never from the C call


def compact_lattice_rescore_raw(csrs, loglikes, row_offsets, tid2pdf):
    """kh_rescore_compact_lattice on CSR dicts (compact_lattice_align_csr: top-sorted, with the strings).  loglikes: DEVICE
    frame x pdf matrix, lattice i's frames in rows row_offsets[i] .. [i + 1]; tid2pdf: num_tids + 1 entries indexed by
    transition-id.  Returns (status [n] of RESCORE_*, utt_len [n], arc_acoustic, final_acoustic: per lattice the new float32
    arrays in CSR order - the old bits where the status is not RESCORE_OK)."""
    n = len(csrs)
    if n == 0:
        raise KhError("compact_lattice_rescore: no lattices")
    if loglikes.dim() != 2 or loglikes.dtype != torch.float32 or not loglikes.is_cuda or loglikes.stride(1) != 1:
        raise KhError("compact_lattice_rescore: loglikes must be a float32 device matrix with unit column stride")
    soff, aoff, _, cat = _batch_csr(csrs)
    arc_strings = [x for L in csrs for x in L["arc_string"]]
    final_strings = [x for L in csrs for x in L["final_string"]]
    lens = lambda strs: np.asarray([len(x) for x in strs], np.int64)
    aso = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens(arc_strings))]).astype(np.int64))
    fso = np.ascontiguousarray((np.concatenate([[0], np.cumsum(lens(final_strings))]) + aso[-1]).astype(np.int64))
    strings = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in arc_strings + final_strings] +
                                                  [np.zeros(0, np.int32)]))
    starts = np.ascontiguousarray(np.asarray([int(L.get("start", 0)) for L in csrs], np.int32))
    ns, a, fg, fa = cat("arc_nextstate", np.int32), cat("arc_acoustic", np.float32), cat("final_graph", np.float32), cat("final_acoustic", np.float32)
    a, fa = a.copy(), fa.copy()
    t2p = np.ascontiguousarray(np.asarray(tid2pdf).astype(np.int32).reshape(-1))
    rows = np.ascontiguousarray(np.asarray(row_offsets).astype(np.int32).reshape(-1))
    if len(rows) != n + 1 or len(t2p) < 2:
        raise KhError("compact_lattice_rescore: row_offsets needs one entry per lattice and one more; tid2pdf num_tids + 1")
    status, utt_len = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ip, fp, lp = capi.c_int32_p, capi.c_float_p, capi.c_int64_p
    ptr = lambda x, t: x.ctypes.data_as(t)
    check(lib().kh_rescore_compact_lattice(
        n, ptr(soff, ip), ptr(starts, ip), ptr(aoff, lp), ptr(ns, ip), ptr(a, fp), ptr(aso, lp), ptr(fg, fp), ptr(fa, fp),
        ptr(fso, lp), ptr(strings, ip), len(strings), _p(loglikes), _dim(loglikes), ptr(rows, ip), len(t2p) - 1, ptr(t2p, ip),
        ptr(status, ip), ptr(utt_len, ip)))
    arcs = [a[int(aoff[soff[i]]):int(aoff[soff[i + 1]])].copy() for i in range(n)]
    finals = [fa[int(soff[i]):int(soff[i + 1])].copy() for i in range(n)]
    return status, utt_len, arcs, finals


def compact_lattice_rescore(clats, loglikes, row_offsets, tid2pdf):
    """RescoreCompactLattice (lat/lattice-functions.cc:1163-1290, 1297-1304) for a batch of CompactLattices (dicts of
    kaldi_io.read_compact_lattice, with the strings) in ONE call; loglikes, row_offsets, tid2pdf as
    compact_lattice_rescore_raw takes them.  Returns per lattice dict(status [RESCORE_*], utt_len, clat): clat = the rescored
    lattice in the same dict layout and in the TOP-SORTED numbering - the reference sorts its argument in place (:1173-1178,
    compact_lattice_top_order) and that is what gmm-rescore-lattice writes - or None where the status is not RESCORE_OK.
    RESCORE_CYCLIC: the sort failed ("Cycles detected in lattice.")."""
    csrs, cyclic = [], []
    for c in clats:
        try:
            csrs.append(compact_lattice_align_csr(c))
            cyclic.append(False)
        except KhError as e:
            if "cycles found" not in str(e):
                raise
            csrs.append(compact_lattice_align_csr(dict(n_states=0)))
            cyclic.append(True)
    status, utt_len, arcs, finals = compact_lattice_rescore_raw(csrs, loglikes, row_offsets, tid2pdf)
    out = []
    for i, L in enumerate(csrs):
        if cyclic[i]:
            out.append(dict(status=RESCORE_CYCLIC, utt_len=0, clat=None))
            continue
        c = None
        if status[i] == RESCORE_OK:
            n = int(L["n_states"])
            c = dict(n_states=n, start=int(L["start"]),
                     arc_src=np.repeat(np.arange(n, dtype=np.int32), np.diff(np.asarray(L["arc_offsets"], np.int64))),
                     arc_dst=np.asarray(L["arc_nextstate"], np.int32).copy(), arc_label=np.asarray(L["arc_label"], np.int32).copy(),
                     arc_g=np.asarray(L["arc_graph"], np.float32).copy(), arc_a=arcs[i], arc_string=list(L["arc_string"]),
                     final_g=np.asarray(L["final_graph"], np.float32).copy(), final_a=finals[i],
                     final_string=list(L["final_string"]), complete=True)
        out.append(dict(status=int(status[i]), utt_len=int(utt_len[i]), clat=c))
    return out


def gmm_rescore_compact_lattices(am, feats, utt_row_offsets, clats, tid2pdf, batch_frames=0):
    """gmm-rescore-lattice's inner call (gmmbin/gmm-rescore-lattice.cc:86-89) for a batch: DecodableAmDiagGmm is unscaled
    and prunes at its default -1.0 (gmm/decodable-am-diag-gmm.h), so the scores are am.pdf_log_likelihoods(feats,
    log_sum_exp_prune=-1.0) - the dense frame x pdf matrix, which the fused scorer fills faster than a list of the (frame,
    pdf) pairs the lattices use could be built.  feats: DEVICE matrix, lattice i's frames in rows utt_row_offsets[i] ..
    [i + 1].  batch_frames > 0 bounds that matrix: consecutive lattices are scored and rescored in groups of at most that
    many frames (one lattice always runs).  Returns compact_lattice_rescore's list."""
    n = len(clats)
    rows = np.asarray(utt_row_offsets).astype(np.int64).reshape(-1)
    if n == 0 or len(rows) != n + 1 or np.any(np.diff(rows) < 0) or rows[0] < 0 or rows[-1] > feats.shape[0]:
        raise KhError("gmm_rescore_compact_lattices: utt_row_offsets needs one ascending entry per lattice and one more, within feats")
    out, i = [], 0
    while i < n:
        j = i + 1
        while j < n and batch_frames > 0 and rows[j + 1] - rows[i] <= batch_frames:
            j += 1
        if batch_frames <= 0:
            j = n
        r0, r1 = int(rows[i]), int(rows[j])
        if r1 > r0:
            ll = am.pdf_log_likelihoods(feats[r0:r1], log_sum_exp_prune=-1.0)
        else:       # no frames at all: every lattice with a transition-id comes back RESCORE_FEATURES_TOO_SHORT
            ll = torch.zeros((1, am.num_pdfs), dtype=torch.float32, device=feats.device)
        out.extend(compact_lattice_rescore(clats[i:j], ll, rows[i:j + 1] - r0, tid2pdf))
        i = j
    return out


def compact_lattice_rescore_last_timings():
    """Milliseconds the last compact_lattice_rescore_raw call of this thread spent in host preparation / uploads / kernels /
    downloads, in the whole C call, and the number of kernel launches and of items rescored one per thread and one per wave."""
    return _timings(lib().kh_rescore_compact_lattice_last_timings, _MS5, ("launches", "thread_items", "wave_items"))


ALIGNC_DONE, ALIGNC_NO_FINAL, ALIGNC_NEEDS_ROOM, ALIGNC_TOO_LARGE, ALIGNC_BOUND, ALIGNC_BAD_INPUT = range(6)

_libm = None


def _libm_f(name):
    """expf / logf of the C library: Exp and Log of base/kaldi-math.h for BaseFloat."""
    global _libm
    if _libm is None:
        import ctypes.util
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    fn = getattr(_libm, name)
    fn.restype, fn.argtypes = C.c_float, [C.c_float]
    return lambda x: np.float32(fn(float(x)))


def transition_id_to_state(tmodel):
    """TransitionIdToTransitionState (hmm/transition-model.h:169): transition-states are the triples, numbered from 1, and
    the transition-ids are numbered triple by triple (ComputeDerived :72-98).  Entry 0 unused (0)."""
    out = [0]
    for i, (phone, hmm_state, _) in enumerate(np.asarray(tmodel["triples"]).reshape(-1, 3)):
        out += [i + 1] * len(tmodel["topo"]["entries"][tmodel["topo"]["phone2idx"][int(phone)]][int(hmm_state)][1])
    return np.asarray(out, np.int32)


def non_self_loop_log_probs(tmodel):
    """ComputeDerivedOfProbs (hmm/transition-model.cc:255-272): per transition-state (entry 0 unused) Log(1 - Exp(log-prob of
    the state's self-loop)) in float, 0 without a self-loop, Log(1e-10) where nothing is left."""
    expf, logf = _libm_f("expf"), _libm_f("logf")
    tstate, self_loop = transition_id_to_state(tmodel), np.asarray(tmodel["tid_is_self_loop"], bool)
    log_probs = np.asarray(tmodel["log_probs"], np.float32)
    out = np.zeros(int(tstate.max()) + 1 if len(tstate) > 1 else 1, np.float32)
    for tid in range(1, len(tstate)):
        if self_loop[tid]:
            rest = np.float32(np.float32(1.0) - expf(log_probs[tid]))
            if rest <= 0.0:
                rest = np.float32(1.0e-10)
            out[tstate[tid]] = logf(rest)
    return out


def add_transition_probs(graph, tmodel, transition_scale, self_loop_scale):
    """AddTransitionProbs (hmm/hmm-utils.cc:776-830) with an empty list of disambiguation symbols, as gmm-align-compiled
    and nnet-align-compiled call it: a copy of `graph` (the dict of kaldi_io.read_fst) whose arcs with a transition-id carry
    weight - scaled log-prob; float arithmetic in the reference's order.  An ilabel outside 0..NumTransitionIds is an error
    (:821-826)."""
    log_probs = np.asarray(tmodel["log_probs"], np.float32)
    num_tids = len(log_probs) - 1
    ts, sl = np.float32(transition_scale), np.float32(self_loop_scale)
    tstate, self_loop = transition_id_to_state(tmodel), np.asarray(tmodel["tid_is_self_loop"], bool)
    il = np.asarray(graph["ilabel"], np.int32)
    bad = il[(il < 0) | (il > num_tids)]
    if len(bad):
        raise KhError("AddTransitionProbs: invalid symbol %d on graph input side." % int(bad[0]))
    scaled = np.zeros(num_tids + 1, np.float32)
    if ts == sl:
        scaled[1:] = log_probs[1:] * ts                                                     # :780-781
    else:
        nsl = non_self_loop_log_probs(tmodel)
        for tid in range(1, num_tids + 1):
            if self_loop[tid]:
                scaled[tid] = sl * log_probs[tid]                                           # :783-784
            else:
                rest = nsl[tstate[tid]]
                ignoring = np.float32(log_probs[tid] - rest)                                # transition-model.cc:333-337
                scaled[tid] = np.float32(np.float32(sl * rest) + np.float32(ts * ignoring))   # :787-788
    out = dict(graph)
    w = np.asarray(graph["weight"], np.float32).copy()
    emit = il != 0
    w[emit] = w[emit] + (-scaled[il[emit]])                                                 # Times :820
    out["weight"] = w
    return out


def modify_graph_for_careful_alignment(graph):
    """ModifyGraphForCarefulAlignment (decoder/decoder-wrappers.cc:393-420) on the dict of kaldi_io.read_fst.  The
    reference concatenates the graph with a copy of itself that has no final weights and a new start state, final with
    weight One, in front (an eps arc of weight One to the copy's old start).  fst::Concat gives every final state of the
    left side an eps arc with its final weight to the right side's start and takes its final weight away.  Here: states
    0..S-1 the graph, S..2S-1 the copy, 2S the new state - the only final one.  (The numbering is the library's own; only
    labels leave the alignment.)"""
    S = int(graph["num_states"])
    if S == 0:
        return dict(graph)
    off = np.asarray(graph["arc_offsets"], np.int64)
    il, ol = np.asarray(graph["ilabel"], np.int32), np.asarray(graph["olabel"], np.int32)
    w, ns = np.asarray(graph["weight"], np.float32), np.asarray(graph["nextstate"], np.int32)
    fin = np.asarray(graph["final"], np.float32)
    is_final = fin != np.float32(np.inf)
    pre = 2 * S
    n_il, n_ol, n_w, n_ns, n_off = [], [], [], [], [0]
    for s in range(S):                                   # the graph: its arcs, then the arc that Concat adds
        a0, a1 = int(off[s]), int(off[s + 1])
        n_il.append(il[a0:a1]); n_ol.append(ol[a0:a1]); n_w.append(w[a0:a1]); n_ns.append(ns[a0:a1])
        if is_final[s]:
            n_il.append(np.zeros(1, np.int32)); n_ol.append(np.zeros(1, np.int32)); n_w.append(fin[s:s + 1]); n_ns.append(np.asarray([pre], np.int32))
        n_off.append(n_off[-1] + (a1 - a0) + int(is_final[s]))
    for s in range(S):                                   # the copy
        a0, a1 = int(off[s]), int(off[s + 1])
        n_il.append(il[a0:a1]); n_ol.append(ol[a0:a1]); n_w.append(w[a0:a1]); n_ns.append(ns[a0:a1] + S)
        n_off.append(n_off[-1] + (a1 - a0))
    n_il.append(np.zeros(1, np.int32)); n_ol.append(np.zeros(1, np.int32)); n_w.append(np.zeros(1, np.float32))
    n_ns.append(np.asarray([S + int(graph["start"])], np.int32))
    n_off.append(n_off[-1] + 1)
    final = np.full(2 * S + 1, np.inf, np.float32)
    final[pre] = 0.0
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt))
    out = dict(graph)
    out.update(num_states=2 * S + 1, start=int(graph["start"]), arc_offsets=np.asarray(n_off, np.int64), ilabel=cat(n_il, np.int32),
               olabel=cat(n_ol, np.int32), weight=cat(n_w, np.float32), nextstate=cat(n_ns, np.int32), final=final)
    return out


def align_compiled_pack(graphs):
    """The graph arguments of kh_align_compiled: the CSR dicts of kaldi_io.read_fst concatenated."""
    n = len(graphs)
    soff = np.zeros(n + 1, np.int32)
    soff[1:] = np.cumsum([int(g["num_states"]) for g in graphs])
    aoff, base = [np.zeros(1, np.int64)], 0
    for g in graphs:
        o = np.asarray(g["arc_offsets"], np.int64).reshape(-1)
        if len(o) != int(g["num_states"]) + 1:
            raise KhError("align_compiled: a graph's arc_offsets do not have num_states + 1 entries")
        aoff.append(o[1:] + base)
        base += int(o[-1]) if len(o) else 0
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(g[k], dt).reshape(-1) for g in graphs] + [np.zeros(0, dt)]))
    A = dict(state_offsets=soff, arc_offsets=np.ascontiguousarray(np.concatenate(aoff)),
             start=np.ascontiguousarray(np.asarray([int(g["start"]) for g in graphs], np.int32)), ilabel=cat("ilabel", np.int32),
             olabel=cat("olabel", np.int32), weight=cat("weight", np.float32), nextstate=cat("nextstate", np.int32),
             final=cat("final", np.float32))
    for k in ("ilabel", "olabel", "weight", "nextstate"):
        if len(A[k]) != base:
            raise KhError("align_compiled: %d entries of %s for %d arcs" % (len(A[k]), k, base))
    if len(A["final"]) != int(soff[-1]):
        raise KhError("align_compiled: %d final weights for %d states" % (len(A["final"]), int(soff[-1])))
    return A


def align_compiled_call(A, loglikes, row_offsets, tid2pdf, beam, min_active, beam_delta, room):
    """One kh_align_compiled call on align_compiled_pack's arrays; loglikes a 2-D float32 device tensor, room = path room
    per utterance.  Returns dict(status, cost, path_len, path_offsets, ilabel, olabel, graph, acoustic)."""
    n = len(A["start"])
    _dim(loglikes)
    ro = np.ascontiguousarray(np.asarray(row_offsets, np.int32).reshape(-1))
    if len(ro) != n + 1:
        raise KhError("align_compiled: %d row offsets for %d utterances" % (len(ro), n))
    t2p = None if tid2pdf is None else np.ascontiguousarray(np.asarray(tid2pdf, np.int32).reshape(-1))
    n_tid = len(t2p) if t2p is not None else int(loglikes.shape[1]) + 1
    po = np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.asarray(room, np.int64).reshape(n))]).astype(np.int64))
    status, plen, best, cost = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    m = max(int(po[-1]), 1)
    p_il, p_ol, p_g, p_a = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.float32), np.zeros(m, np.float32)
    ip, fp, lp = capi.c_int32_p, capi.c_float_p, capi.c_int64_p
    ptr = lambda x, t: x.ctypes.data_as(t)
    check(lib().kh_align_compiled(
        n, ptr(A["state_offsets"], ip), ptr(A["arc_offsets"], lp), ptr(A["start"], ip), ptr(A["ilabel"], ip), ptr(A["olabel"], ip),
        ptr(A["weight"], fp), ptr(A["nextstate"], ip), ptr(A["final"], fp), n_tid, None if t2p is None else ptr(t2p, ip),
        _p(loglikes), int(loglikes.shape[0]), int(loglikes.shape[1]), int(loglikes.stride(0)) if loglikes.shape[0] > 1 else int(loglikes.shape[1]),
        ptr(ro, ip), float(beam), int(min_active), float(beam_delta), ptr(po, lp), ptr(status, ip), ptr(cost, capi.c_double_p),
        ptr(best, ip), ptr(plen, ip), ptr(p_il, ip), ptr(p_ol, ip), ptr(p_g, fp), ptr(p_a, fp)))
    return dict(status=status, cost=cost, best_state=best, path_len=plen, path_offsets=po, ilabel=p_il, olabel=p_ol, graph=p_g, acoustic=p_a)


def align_compiled_raw(graphs, loglikes, row_offsets, tid2pdf, beam, min_active=20, beam_delta=0.5, workspace_limit=None,
                       path_room=None):
    """One Decode() per utterance (kh_align_compiled) and, for the utterances whose path did not fit the room, one more call
    with the room they named.  path_room: None = 2 x frames + 16 arcs per utterance (a training graph has two or three eps arcs per word), or a
    number per utterance.  Returns per
    utterance dict(status, cost, best_state, path [(ilabel, olabel, graph_cost, ac_cost)], path_len)."""
    n = len(graphs)
    if n == 0:
        raise KhError("align_compiled: no utterances")
    ro = np.asarray(row_offsets, np.int64).reshape(-1)
    frames = np.diff(ro)
    room = 2 * frames + 16 if path_room is None else np.broadcast_to(np.asarray(path_room, np.int64), (n,))
    with _workspace_limit(lib().kh_align_compiled_set_workspace_limit, workspace_limit):
        out = [None] * n
        todo = list(range(n))
        for attempt in range(2):
            A = align_compiled_pack([graphs[u] for u in todo])
            sub_ro = np.concatenate([[0], np.cumsum(frames[todo])])
            if len(todo) == n:
                ll, sub_ro = loglikes, ro
            else:   # the rows of the utterances that go again, gathered (torch owns the memory; nothing is computed)
                ll = torch.cat([loglikes[int(ro[u]):int(ro[u + 1])] for u in todo]) if int(sub_ro[-1]) > 0 else loglikes[:0]
                ll = ll.contiguous()
            R = align_compiled_call(A, ll, sub_ro, tid2pdf, beam, min_active, beam_delta, np.asarray(room)[todo])
            again = []
            for k, u in enumerate(todo):
                st, p0, ln = int(R["status"][k]), int(R["path_offsets"][k]), int(R["path_len"][k])
                if st == ALIGNC_NEEDS_ROOM and attempt == 0:
                    room = np.array(room, np.int64)
                    room[u] = ln
                    again.append(u)
                    continue
                path = []
                if st == ALIGNC_DONE:
                    path = [(int(R["ilabel"][p0 + i]), int(R["olabel"][p0 + i]), R["graph"][p0 + i], R["acoustic"][p0 + i]) for i in range(ln)]
                out[u] = dict(status=st, cost=float(R["cost"][k]), best_state=int(R["best_state"][k]), path=path, path_len=ln)
            todo = again
            if not todo:
                break
    return out


def linear_symbol_sequence(path, final_weight):
    """GetLinearSymbolSequence (fstext/fstext-utils-inl.h) on the linear best path: the nonzero ilabels, the nonzero olabels
    and the Times of the arcs' LatticeWeights in path order with the final weight last, float sums."""
    g = a = np.float32(0.0)
    for (_, _, pg, pa) in path:
        g, a = np.float32(g + np.float32(pg)), np.float32(a + np.float32(pa))
    g = np.float32(g + np.float32(final_weight))
    return [x[0] for x in path if x[0] != 0], [x[1] for x in path if x[1] != 0], (g, a)


def align_compiled(graphs, loglikes, row_offsets, tid2pdf, beam, retry_beam=0.0, careful=False, min_active=20, beam_delta=0.5,
                   workspace_limit=None, path_room=None):
    """AlignUtteranceWrapper (decoder/decoder-wrappers.cc:423-505) for a batch: graphs = the utterances' decoding graphs
    (dicts of kaldi_io.read_fst, transition probabilities already added), loglikes = the scaled log-likelihoods of all
    utterances as one 2-D float32 device tensor, utterance u at rows row_offsets[u]..row_offsets[u+1], tid2pdf indexed by
    transition-id (None = ilabel - 1).  The search is FasterDecoder by the rule of include/kaldi_hip.h at kh_align_compiled.
    The utterances that reach no final state with `beam` are searched once more with `retry_beam` (0 = not), in a second
    call over them alone.  Returns per utterance dict(status [ALIGNC_*], retried, alignment, words, cost [the double total],
    weight [(graph, acoustic) floats, the final weight in graph], like [float -(graph + acoustic), the value of the scores
    table], path)."""
    beam, retry_beam = float(beam), float(retry_beam)
    if (retry_beam != 0 and retry_beam <= beam) or beam <= 0.0:                           # :439-443
        raise KhError("Beams do not make sense: beam %g, retry-beam %g" % (beam, retry_beam))
    if careful:
        graphs = [modify_graph_for_careful_alignment(g) for g in graphs]
    res = align_compiled_raw(graphs, loglikes, row_offsets, tid2pdf, beam, min_active, beam_delta, workspace_limit, path_room)
    for r in res:
        r["retried"] = False
    again = [u for u, r in enumerate(res) if r["status"] == ALIGNC_NO_FINAL]
    if again and retry_beam != 0:                                                          # :464-472
        ro = np.asarray(row_offsets, np.int64).reshape(-1)
        frames = np.diff(ro)[again]
        sub_ro = np.concatenate([[0], np.cumsum(frames)])
        ll = torch.cat([loglikes[int(ro[u]):int(ro[u + 1])] for u in again]).contiguous() if int(sub_ro[-1]) > 0 else loglikes[:0]
        room = None if path_room is None else np.broadcast_to(np.asarray(path_room, np.int64), (len(graphs),))[again]
        sub = align_compiled_raw([graphs[u] for u in again], ll, sub_ro, tid2pdf, retry_beam, min_active, beam_delta, workspace_limit, room)
        for u, r in zip(again, sub):
            r["retried"] = True
            res[u] = r
    for u, r in enumerate(res):
        r["alignment"], r["words"], r["weight"], r["like"] = [], [], None, None
        if r["status"] == ALIGNC_DONE:
            r["alignment"], r["words"], r["weight"] = linear_symbol_sequence(r["path"], graphs[u]["final"][r["best_state"]])
            r["like"] = np.float32(-np.float32(r["weight"][0] + r["weight"][1]))
    return res


def align_compiled_set_lds_states(max_states):
    """Utterances with more states than this keep their token costs in the call's workspace instead of LDS (calling
    thread; at most 3584, the default; 0 = always the workspace).  A test and measurement aid."""
    check(lib().kh_align_compiled_set_lds_states(int(max_states)))


def align_compiled_last_timings():
    """Milliseconds the last kh_align_compiled call of this thread spent in host preparation / uploads / kernels / downloads
    and in the whole call, and the number of kernel launches, of utterances whose costs lay in the workspace and of
    utterances launched."""
    return _timings(lib().kh_align_compiled_last_timings, _MS5, ("launches", "workspace_cost_utts", "utts_launched"))


def rescore_lattice(lats, loglikes, utt_row_offsets, tid2pdf=None):
    """RescoreLattice (lat/lattice-functions.cc:1307-1358) for a batch: loglikes = device
    matrix (rows of lattice i at utt_row_offsets[i]...).  Returns the new arc_acoustic arrays."""
    n, soff, aoff, il, ns, g, a, fin = _cat_lattices(lats)
    a = a.copy()
    off = np.ascontiguousarray(utt_row_offsets, np.int32)
    ip, fp = capi.c_int32_p, capi.c_float_p
    check(lib().kh_rescore_lattice(n, soff.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), il.ctypes.data_as(ip),
                                   ns.ctypes.data_as(ip), a.ctypes.data_as(fp), _p(loglikes), _dim(loglikes).stride,
                                   off.ctypes.data_as(ip), _p(tid2pdf) if tid2pdf is not None else None))
    return [a[int(aoff[soff[i]]):int(aoff[soff[i + 1]])].copy() for i in range(n)]


def comp_objf_and_deriv(deriv, sv_labels, output):
    """CuMatrix::CompObjfAndDeriv (cu-matrix.cc:1198-1248): deriv.CompObjfAndDeriv(sv_labels,
    output, &tot_objf, &tot_weight); sv_labels = [(row, column, weight), ...]."""
    r = np.ascontiguousarray([x[0] for x in sv_labels], np.int32)
    c = np.ascontiguousarray([x[1] for x in sv_labels], np.int32)
    w = np.ascontiguousarray([x[2] for x in sv_labels], np.float32)
    objf, wt = C.c_float(), C.c_float()
    check(lib().kh_comp_objf_and_deriv(len(r), r.ctypes.data_as(capi.c_int32_p), c.ctypes.data_as(capi.c_int32_p),
                                       w.ctypes.data_as(capi.c_float_p), _p(output), _dim(output), _p(deriv), _dim(deriv),
                                       C.byref(objf), C.byref(wt)))
    return objf.value, wt.value


# ---- Posterior algebra of hmm/posterior.cc used by LatticeForwardBackwardMmi (host lists,
# as in the reference).  A Posterior is a list over frames of [(id, weight), ...].
def alignment_to_posterior(ali):
    """AlignmentToPosterior hmm/posterior.cc:276-285."""
    return [[(int(t), 1.0)] for t in ali]


def scale_posterior(scale, post):
    """ScalePosterior hmm/posterior.cc:204-218 (scale == 0 clears the frames)."""
    if scale == 0.0:
        return [[] for _ in post]
    return [[(i, float(np.float32(np.float32(w) * np.float32(scale)))) for i, w in fr] for fr in post]


def convert_posterior_to_pdfs(tid2pdf, post):
    """ConvertPosteriorToPdfs hmm/posterior.cc:308-332 (entries of a frame in ascending pdf
    order here; the reference's order is that of an unordered_map)."""
    out = []
    for fr in post:
        acc = {}
        for tid, w in fr:
            pdf = int(tid2pdf[tid])
            acc[pdf] = np.float32(acc[pdf] + np.float32(w)) if pdf in acc else np.float32(w)
        out.append([(k, float(v)) for k, v in sorted(acc.items()) if v != 0.0])
    return out


def merge_posteriors(post1, post2, merge, drop_frames):
    """MergePosteriors hmm/posterior.cc:244-274; returns (post, num_disjoint)."""
    assert len(post1) == len(post2)
    out, num_disjoint = [], 0
    for a, b in zip(post1, post2):
        fr = list(a) + list(b)
        if merge:  # MergePairVectorSumming: sort on the id, sum equal ids, drop zeros
            fr.sort(key=lambda x: x[0])
            merged = []
            for i, w in fr:
                if merged and merged[-1][0] == i:
                    merged[-1] = (i, float(np.float32(np.float32(merged[-1][1]) + np.float32(w))))
                else:
                    merged.append((i, float(np.float32(w))))
            fr = [(i, w) for i, w in merged if w != 0.0]
        else:
            fr.sort()
        if not ({i for i, _ in a} & {i for i, _ in b}):  # PosteriorEntriesAreDisjoint :220-241
            num_disjoint += 1
            if drop_frames:
                fr = []
        out.append(fr)
    return out, num_disjoint


def lattice_forward_backward_mmi(lats, tid2pdf, num_alis, drop_frames, convert_to_pdf_ids, cancel):
    """LatticeForwardBackwardMmi (lat/lattice-functions.cc:1361-1396) for a batch: the
    denominator forward-backward on the GPU, the posterior algebra on the host as in the
    reference.  Returns per lattice dict(post, tot_like)."""
    fb = lattice_forward_backward(lats)
    out = []
    for r, ali in zip(fb, num_alis):
        den_post = scale_posterior(-1.0, r["post"])
        num_post = alignment_to_posterior(ali)
        if convert_to_pdf_ids:
            num_post = convert_posterior_to_pdfs(tid2pdf, num_post)
            den_post = convert_posterior_to_pdfs(tid2pdf, den_post)
        post, _ = merge_posteriors(num_post, den_post, cancel, drop_frames)
        out.append(dict(post=post, tot_like=r["tot_like"]))
    return out


# ---------------------------------------------------------------- config 5: discriminative pass
def _lookup_values(M, rows, cols):
    """CuMatrix::Lookup (cu-matrix.cc:2327) for index arrays."""
    pairs = np.empty((len(rows), 2), np.int32)
    pairs[:, 0] = rows
    pairs[:, 1] = cols
    out = lookup(M, pairs)
    synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _merge_keyed(rows, cols, weights, n_rows=None):
    """Sum float32 weights per (row, col), drop exact zeros; keys sorted (MergePairVectorSumming
    per frame, util/stl-utils.h:303-322, for all frames at once: kh_merge_pair_vector_summing)."""
    n = len(rows)
    if n == 0:
        return rows.astype(np.int64), cols.astype(np.int64), weights.astype(np.float32)
    r = np.ascontiguousarray(rows, np.int32)
    c = np.ascontiguousarray(cols, np.int32)
    w = np.ascontiguousarray(weights, np.float32)
    if n_rows is None:
        n_rows = int(r.max()) + 1
    orow, ocol, ow = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    n_out = C.c_int64()
    ip, fp = capi.c_int32_p, capi.c_float_p
    check(lib().kh_merge_pair_vector_summing(n, r.ctypes.data_as(ip), c.ctypes.data_as(ip), w.ctypes.data_as(fp), int(n_rows),
                                             orow.ctypes.data_as(ip), ocol.ctypes.data_as(ip), ow.ctypes.data_as(fp),
                                             C.byref(n_out)))
    m = n_out.value
    return orow[:m].astype(np.int64), ocol[:m].astype(np.int64), ow[:m]


def sort_pairs64(keys, vals, lo_bits, hi_bits):
    """kh_sort_pairs64: the device radix sort of the discriminative call by itself.  keys uint64 [n], vals int32 [n] (host)
    -> (keys, vals) in the stable order of the keys' low lo_bits bits and the hi_bits bits from bit 32 on."""
    k = np.ascontiguousarray(keys, np.uint64)
    v = np.ascontiguousarray(vals, np.int32)
    if k.ndim != 1 or k.shape != v.shape:
        raise KhError("sort_pairs64: one payload per key")
    ko, vo = np.empty_like(k), np.empty_like(v)
    check(lib().kh_sort_pairs64(len(k), k.ctypes.data_as(capi.c_uint64_p), v.ctypes.data_as(capi.c_int32_p), int(lo_bits), int(hi_bits),
                                ko.ctypes.data_as(capi.c_uint64_p), vo.ctypes.data_as(capi.c_int32_p)))
    return ko, vo


class DiscriminativeCall:
    """A discriminative_lattice_computations(..., begin=True) in flight: its device work is queued on a stream of its own
    (kh_discriminative_lattice_computations_begin); end() waits for it and returns what the plain call returns."""

    def __init__(self, handle, out, deriv, Ts, weights):
        self._h, self.output, self.deriv, self._Ts, self._w = handle, out, deriv, Ts, weights

    def end(self):
        if self._h is None:
            raise KhError("DiscriminativeCall.end() called twice")
        st = np.zeros(5)
        h, self._h = self._h, None
        check(lib().kh_discriminative_lattice_computations_end(h, st.ctypes.data_as(capi.c_double_p)))
        stats = dict(tot_t=float(self._Ts.sum()), tot_t_weighted=float((self._Ts * self._w).sum()), tot_num_count=float(st[0]),
                     tot_num_objf=float(st[1]), tot_den_objf=float(st[2]))
        return dict(stats=stats, deriv=self.deriv, output=self.output, objf=float(st[3]), weight=float(st[4]))

    def __del__(self):
        try:
            if self._h is not None:
                lib().kh_discriminative_lattice_computations_end(self._h, np.zeros(5).ctypes.data_as(capi.c_double_p))
                self._h = None
        except Exception:
            pass


def discriminative_lattice_computations(nnet, priors, tid2pdf, egs, criterion="smbr", acoustic_scale=0.1,
                                        drop_frames=False, one_silence_class=False, tid2phone=None,
                                        silence_phones=(), den_lats=None, begin=False):
    """NnetDiscriminativeUpdater::Propagate + LatticeComputations
    (nnet2/nnet-compute-discriminative.cc:150-321) for a BATCH of examples, as one pipeline
    on the device: network forward -> CuMatrix::Lookup of the posteriors the numerator
    alignment and the denominator lattice arcs need (:196-226) -> scaled pseudo log-likelihoods
    log(post / prior) x acoustic_scale with the 1e-20 floor (:231-247) written into the lattice
    (:259-277) -> MMI / sMBR / MPFE forward-backward (GetDiscriminativePosteriors :324-343) ->
    the Posterior algebra of hmm/posterior.cc + ScalePosterior(weight) -> CompObjfAndDeriv (:279-316);
    everything behind the forward pass is ONE library call, kh_discriminative_lattice_computations
    (the host hands over the lattices and the alignments, nothing comes back but five numbers).
    (--boost is not supported.)

    egs: list of dict(feats = device [T + left + right, D] with exactly the network's context,
    num_ali = int32 [T], den_lat = top-sorted CSR lattice (lattice_to_csr), weight = float).
    den_lats: optionally the examples' lattices already concatenated (cat_lattices(...)), e.g. by the
    data loader's worker - the egs' den_lat entries are then not read.
    Returns dict(stats = NnetDiscriminativeStats fields, deriv = device matrix [sum T, num_pdfs]:
    the derivative at the network output, output = the posteriors).
    begin=True: returns a DiscriminativeCall as soon as the work is queued (the lattice steps on a stream of the call's
    own); launch the NEXT batch's call - its forward pass runs beside this batch's sweeps - then .end() this one."""
    if criterion not in ("mmi", "smbr", "mpfe"):
        raise KhError('criterion must be "mmi", "mpfe" or "smbr"')
    n = len(egs)
    timing = os.environ.get("KH_LATTICE_TIMING") is not None   # host-side split of the call on stderr (tools/time_cfg5.py)
    t_in = time.perf_counter()
    t2p = np.ascontiguousarray(tid2pdf, np.int32)
    pri = np.ascontiguousarray(priors, np.float32)
    Ts = np.array([len(e["num_ali"]) for e in egs], np.int64)
    row_off = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int32)
    # ---- Propagate (:150-175): the examples carry exactly the context the network needs
    feat_rows = np.array([e["feats"].shape[0] for e in egs], np.int64)
    foff = np.concatenate([[0], np.cumsum(feat_rows)]).astype(np.int32)
    feats = torch.cat([e["feats"] for e in egs], 0) if n > 1 else egs[0]["feats"]
    out, out_off = nnet.compute(feats, foff, pad_input=False, wait=False)   # (the lattice call below ends with a wait for the stream)
    t_fwd = time.perf_counter()
    if not np.array_equal(np.diff(np.asarray(out_off)), Ts):
        raise KhError("KALDI_ASSERT(posteriors.NumRows() == num_frames) nnet-compute-discriminative.cc:194")
    if out.shape[1] != len(pri):
        raise KhError("KALDI_ASSERT(num_pdfs == priors.Dim()) :196")
    if criterion != "mmi" and tid2phone is None:
        raise KhError("sMBR / MPFE need the transition-id -> phone map")
    ali = np.ascontiguousarray(np.concatenate([np.asarray(e["num_ali"], np.int32) for e in egs]), np.int32)
    weights = np.array([float(e.get("weight", 1.0)) for e in egs], np.float32)
    t2ph = np.ascontiguousarray(tid2phone, np.int32) if tid2phone is not None else None
    sil = np.ascontiguousarray(sorted(silence_phones), np.int32)
    deriv = torch.empty_like(out)
    st = np.zeros(5)
    ip, fp = capi.c_int32_p, capi.c_float_p
    tail = (ali.ctypes.data_as(ip), row_off.ctypes.data_as(ip),
            weights.ctypes.data_as(fp), t2p.ctypes.data_as(ip), t2ph.ctypes.data_as(ip) if t2ph is not None else None, len(t2p) - 1,
            sil.ctypes.data_as(ip), len(sil), {"mmi": 0, "smbr": 1, "mpfe": 2}[criterion], float(acoustic_scale), int(bool(drop_frames)),
            int(bool(one_silence_class)), pri.ctypes.data_as(fp), _p(out), _dim(out), _p(deriv), _dim(deriv),
            st.ctypes.data_as(capi.c_double_p))
    if den_lats is None:
        # the lattices as the examples hold them: the library assembles the batch (host threads, pinned memory) and prepares
        # it on the device beside the forward pass launched above, which nobody has waited for yet
        keep, cols = [], []
        for key, dt in (("arc_offsets", np.int64), ("arc_ilabel", np.int32), ("arc_nextstate", np.int32), ("arc_graph", np.float32),
                        ("arc_acoustic", np.float32), ("state_final", np.float32)):
            arrs = [np.ascontiguousarray(e["den_lat"][key], dt) for e in egs]
            keep.append(arrs)
            cols.append(np.fromiter((x.__array_interface__["data"][0] for x in arrs), np.uint64, n))
        nst = np.fromiter((e["den_lat"]["n_states"] for e in egs), np.int32, n)
        lens = [np.fromiter((x.size if x.ndim == 1 else -1 for x in arrs), np.int64, n) for arrs in keep]
        na = np.fromiter((int(x[-1]) if x.size else -1 for x in keep[0]), np.int64, n)
        good = (lens[0] == nst + 1) & (lens[5] == nst)
        for k in range(1, 5):
            good &= lens[k] == na
        if not good.all():
            raise KhError("example %d: the arrays of den_lat do not have the lengths n_states / arc_offsets give" % int(np.argmin(good)))
        vp = C.c_void_p
        if timing:
            sys.stderr.write("[api timing] forward launched after %.2f ms, lattice arrays listed after %.2f ms\n"
                             % ((t_fwd - t_in) * 1e3, (time.perf_counter() - t_in) * 1e3))
        if begin:
            h = vp()
            check(lib().kh_discriminative_lattice_computations_begin(
                n, nst.ctypes.data_as(ip), *[c.ctypes.data_as(vp) for c in cols], *tail[:-1], C.byref(h)))
            return DiscriminativeCall(h, out, deriv, Ts, weights)   # (the host arrays have been copied or uploaded)
        check(lib().kh_discriminative_lattice_computations_parts(
            n, nst.ctypes.data_as(ip), *[c.ctypes.data_as(vp) for c in cols], *tail))
        del keep
    else:
        if begin:
            raise KhError("begin=True takes the lattices by example (den_lats=None)")
        nl, soff, aoff, il, ns, g, a, fin = den_lats
        if nl != n:
            raise KhError("one denominator lattice per example")
        check(lib().kh_discriminative_lattice_computations(
            nl, soff.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), il.ctypes.data_as(ip), ns.ctypes.data_as(ip),
            g.ctypes.data_as(fp), a.ctypes.data_as(fp), fin.ctypes.data_as(fp), *tail))
    stats = dict(tot_t=float(Ts.sum()), tot_t_weighted=float((Ts * weights).sum()), tot_num_count=float(st[0]),
                 tot_num_objf=float(st[1]), tot_den_objf=float(st[2]))
    return dict(stats=stats, deriv=deriv, output=out, objf=float(st[3]), weight=float(st[4]))


def cat_lattices(lats):
    """The batch form of top-sorted CSR lattices the library's lattice calls take (what a data loader can prepare ahead)."""
    return _cat_lattices(lats)


def lattice_forward_backward_mpe_raw(lats, tid2phone, tid2pdf, silence_phones, num_alis, criterion, one_silence_class):
    """kh_lattice_forward_backward_mpe for a batch, arrays only (no per-frame Python lists)."""
    n, soff, aoff, il, ns, g, a, fin = _cat_lattices(lats)
    t2ph, t2pdf = np.ascontiguousarray(tid2phone, np.int32), np.ascontiguousarray(tid2pdf, np.int32)
    sil = np.ascontiguousarray(sorted(silence_phones), np.int32)
    ali_off = np.concatenate([[0], np.cumsum([len(x) for x in num_alis])]).astype(np.int32)
    ali = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in num_alis]), np.int32)
    post = np.empty(len(il), np.float32)
    score = np.empty(n)
    ip, fp, dp = capi.c_int32_p, capi.c_float_p, capi.c_double_p
    check(lib().kh_lattice_forward_backward_mpe(
        n, soff.ctypes.data_as(ip), aoff.ctypes.data_as(capi.c_int64_p), il.ctypes.data_as(ip), ns.ctypes.data_as(ip),
        g.ctypes.data_as(fp), a.ctypes.data_as(fp), fin.ctypes.data_as(fp), t2ph.ctypes.data_as(ip),
        t2pdf.ctypes.data_as(ip), len(t2ph) - 1, sil.ctypes.data_as(ip), len(sil), ali.ctypes.data_as(ip),
        ali_off.ctypes.data_as(ip), int(criterion == "mpfe"), int(bool(one_silence_class)), post.ctypes.data_as(fp),
        score.ctypes.data_as(dp), None))
    return dict(arc_post=post, tot_forward_score=score)


# ---------------------------------------------------------------- lattice determinization
def tid_phone_map(tm):
    """What DeterminizeLatticeInsertPhones asks the TransitionModel per transition-id (determinize-lattice-pruned.cc:1335-1338):
    tid_phone[tid] = TransitionIdToPhone(tid) when TransitionIdToHmmState(tid) == 0 and not IsSelfLoop(tid), else 0.
    `tm`: the dict kaldi_io.read_transition_model returns (tid2phone, tid2hmm_state, tid_is_self_loop)."""
    ph = np.asarray(tm["tid2phone"], np.int32)
    keep = (np.asarray(tm["tid2hmm_state"]) == 0) & ~np.asarray(tm["tid_is_self_loop"], bool)
    out = np.where(keep, ph, 0).astype(np.int32)
    out[0] = 0
    return out


def determinize_lattice_pruned(L, beam, delta=2.0 ** -10, max_mem=50000000, tid_phone=None, phone_determinize=None,
                               word_determinize=True, minimize=False):
    """DeterminizeLatticePhonePrunedWrapper (lat/determinize-lattice-pruned.cc:1497-1519; call
    site decoder/decoder-wrappers.cc:264-274) on a raw lattice (get_raw_lattice layout).
    Returns the CompactLattice as a dict: n_states (state 0 = start), arcs sorted by source
    (arc_src, arc_dst, arc_label = word, arc_g, arc_a, arc_string = list of int32 arrays of
    transition-ids), final_g / final_a (+inf for non-final states), final_string, complete
    (False: "Determinization finished earlier than the beam").  Host code, no GPU involved."""
    ip, fp = capi.c_int32_p, capi.c_float_p
    src = np.ascontiguousarray(L["arc_src"], np.int32)
    dst = np.ascontiguousarray(L["arc_dst"], np.int32)
    il = np.ascontiguousarray(L["arc_il"], np.int32)
    ol = np.ascontiguousarray(L["arc_ol"], np.int32)
    g = np.ascontiguousarray(L["arc_g"], np.float32)
    a = np.ascontiguousarray(L["arc_a"], np.float32)
    fin = np.ascontiguousarray(L["state_final"], np.float32)
    if phone_determinize is None:       # the reference's default (true) wherever the transition model's map is given
        phone_determinize = tid_phone is not None
    tp = np.ascontiguousarray(tid_phone, np.int32) if tid_phone is not None else None
    if phone_determinize and tp is None:
        raise KhError("phone_determinize needs tid_phone (api.tid_phone_map of the transition model)")
    h = lib().kh_determinize_lattice_phone_pruned(len(fin), len(src), src.ctypes.data_as(ip), dst.ctypes.data_as(ip),
                                                  il.ctypes.data_as(ip), ol.ctypes.data_as(ip), g.ctypes.data_as(fp),
                                                  a.ctypes.data_as(fp), fin.ctypes.data_as(fp),
                                                  tp.ctypes.data_as(ip) if tp is not None else None, len(tp) if tp is not None else 0,
                                                  float(beam), float(delta), int(max_mem), int(bool(phone_determinize)),
                                                  int(bool(word_determinize)), int(bool(minimize)))
    if not h:
        raise KhError(lib().kh_last_error().decode())
    h = C.c_void_p(h)
    try:
        return _read_compact_lattice(h)
    finally:
        lib().kh_compact_lattice_free(h)


def _read_compact_lattice(h):
    """KhCompactLattice handle -> the dict layout of determinize_lattice_pruned."""
    ip, fp = capi.c_int32_p, capi.c_float_p
    if True:
        n, m, ns_, nf_, comp = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().kh_compact_lattice_sizes(h, C.byref(n), C.byref(m), C.byref(ns_), C.byref(nf_), C.byref(comp)))
        n, m = n.value, m.value
        out = dict(n_states=n, arc_src=np.empty(m, np.int32), arc_dst=np.empty(m, np.int32), arc_label=np.empty(m, np.int32),
                   arc_g=np.empty(m, np.float32), arc_a=np.empty(m, np.float32), final_g=np.empty(n, np.float32),
                   final_a=np.empty(n, np.float32), complete=bool(comp.value))
        aso, fso = np.zeros(m + 1, np.int32), np.zeros(n + 1, np.int32)
        astr, fstr = np.empty(ns_.value, np.int32), np.empty(nf_.value, np.int32)
        check(lib().kh_compact_lattice_get(h, out["arc_src"].ctypes.data_as(ip), out["arc_dst"].ctypes.data_as(ip),
                                           out["arc_label"].ctypes.data_as(ip), out["arc_g"].ctypes.data_as(fp),
                                           out["arc_a"].ctypes.data_as(fp), aso.ctypes.data_as(ip), astr.ctypes.data_as(ip),
                                           out["final_g"].ctypes.data_as(fp), out["final_a"].ctypes.data_as(fp),
                                           fso.ctypes.data_as(ip), fstr.ctypes.data_as(ip)))
        out["arc_string"] = [astr[aso[j]:aso[j + 1]].copy() for j in range(m)]
        out["final_string"] = [fstr[fso[s]:fso[s + 1]].copy() for s in range(n)]
        return out


def host_cpus():
    """CPUs this process may use: the affinity mask, capped by the cgroup's CPU quota (cpu.max; a container that sees 256
    cores and is granted 16 runs 16 threads well and 256 badly - beyond the quota the kernel throttles the whole group)."""
    import os as _os
    n = len(_os.sched_getaffinity(0)) if hasattr(_os, "sched_getaffinity") else (_os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = max(1, min(n, -(-int(q) // int(per))))
    except (OSError, ValueError):
        pass
    return n


def determinize_lattices(lats, beam, delta=2.0 ** -10, max_mem=50000000, num_threads=0, **kw):
    """determinize_lattice_pruned for a batch on host threads (the library call releases the
    GIL; utterances are independent, as the reference's $nj jobs / TaskSequencer threads)."""
    import concurrent.futures
    nt = num_threads if num_threads > 0 else min(len(lats), host_cpus())
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, nt)) as ex:
        return list(ex.map(lambda L: determinize_lattice_pruned(L, beam, delta, max_mem, **kw), lats))


# ---------------------------------------------------------------- iVector extraction (f3)
class OnlineIvectorExtractor:
    """OnlineIvectorExtractionInfo + OnlineIvectorFeature (online2/online-ivector-feature.h:51-134,
    :226-330) in the deterministic mode (no silence weighting, use_most_recent_ivector = false, a
    fresh adaptation state per utterance), batched over utterances.  `info`: lda_mat
    [feat_dim x (spliced dim (+ 1))], global_cmvn_stats [2 x (base_dim + 1)], splice_left/right,
    cmn_window / speaker_frames / global_frames / normalize_mean / normalize_variance
    (OnlineCmvnOptions), the diagonal UBM (ubm_weights, ubm_means, ubm_vars), the IvectorExtractor
    (M [I x D x S], Sigma_inv [I x D x D], prior_offset) and ivector_period, num_gselect, min_post,
    posterior_scale, max_count, num_cg_iters (online-ivector-feature.h:102-107)."""

    def __init__(self, info):
        lda = np.ascontiguousarray(info["lda_mat"], np.float32)
        gs = np.ascontiguousarray(info["global_cmvn_stats"], np.float64)
        M = np.ascontiguousarray(info["M"], np.float64)
        si = np.ascontiguousarray(info["Sigma_inv"], np.float64)
        inv = (1.0 / np.asarray(info["ubm_vars"], np.float64)).astype(np.float32)
        mi = (np.asarray(info["ubm_means"], np.float64) / np.asarray(info["ubm_vars"], np.float64)).astype(np.float32)
        g, bad = gmm_compute_gconsts(info["ubm_weights"], mi, inv)
        if bad:
            raise KhError("DiagGmm::ComputeGconsts: %d bad gconsts in the UBM" % bad)
        cfg = capi.KhIvectorConfig()
        cfg.base_dim = gs.shape[1] - 1
        cfg.splice_left, cfg.splice_right = int(info["splice_left"]), int(info["splice_right"])
        cfg.feat_dim, cfg.lda_cols = lda.shape
        cfg.num_gauss, _, cfg.ivector_dim = M.shape
        if M.shape[1] != cfg.feat_dim or si.shape != (cfg.num_gauss, cfg.feat_dim, cfg.feat_dim) or mi.shape != (cfg.num_gauss, cfg.feat_dim):
            raise KhError("OnlineIvectorExtractionInfo: model dimensions do not match")
        for k in ("cmn_window", "speaker_frames", "global_frames", "normalize_mean", "normalize_variance",
                  "ivector_period", "num_gselect", "num_cg_iters"):
            setattr(cfg, k, int(info[k]))
        for k in ("min_post", "posterior_scale", "max_count", "prior_offset"):
            setattr(cfg, k, float(info[k]))
        # use_most_recent_ivector + greedy_ivector_extractor (--online=false): one estimate per utterance
        cfg.greedy_most_recent = int(bool(info.get("greedy_most_recent", False)))
        self.cfg = cfg
        fp, dp = capi.c_float_p, capi.c_double_p
        self._h = lib().kh_ivector_extractor_create(C.byref(cfg), lda.ctypes.data_as(fp), gs.ctypes.data_as(dp),
                                                    g.ctypes.data_as(fp), mi.ctypes.data_as(fp), inv.ctypes.data_as(fp),
                                                    M.ctypes.data_as(dp), si.ctypes.data_as(dp))
        if not self._h:
            raise KhError(lib().kh_last_error().decode())

    @property
    def ivector_dim(self):
        return self.cfg.ivector_dim

    def state_dim(self):
        return int(lib().kh_ivector_state_dim(self._h))

    def fresh_state(self, n):
        """OnlineIvectorExtractorAdaptationState of n new speakers (online-ivector-feature.h:138-176) in the
        library's layout: CMVN speaker stats [2 (B + 1)], num_frames, prior share of the quadratic diagonal (1),
        linear term [S] (prior_offset in the first dimension), per-Gaussian counts [I]."""
        st = np.zeros((n, self.state_dim()))
        lo = 2 * (self.cfg.base_dim + 1) + 2
        st[:, lo - 1] = 1.0
        st[:, lo] = self.cfg.prior_offset
        return st

    def limit_frames(self, state, max_remembered_frames=1000.0):
        """OnlineIvectorExtractorAdaptationState::LimitFrames (online-ivector-feature.cc:99-117) +
        OnlineIvectorEstimationStats::Scale (ivector-extractor.cc:570-592), in place on [n x state_dim]."""
        B, S = self.cfg.base_dim, self.cfg.ivector_dim
        nc, lo = 2 * (B + 1), 2 * (B + 1) + 2
        mc, po = float(self.cfg.max_count), float(self.cfg.prior_offset)
        for st in state:
            count = np.float32(st[B])
            if count > max_remembered_frames:
                st[:nc] *= float(np.float32(max_remembered_frames) / count)
            lim = float(np.float32(max_remembered_frames) * np.float32(self.cfg.posterior_scale))
            n = st[lo - 2]
            if n > lim:
                scale = lim / n
                st[lo - 2] = n * scale
                st[lo + S:] *= scale                      # the counts: the data part of the quadratic term
                st[lo:lo + S] *= scale
                add = (1.0 - scale) if mc == 0.0 else max(n * scale, mc) / mc - scale * max(n, mc) / mc
                st[lo - 1] = st[lo - 1] * scale + add
                st[lo] += po * add
        return state

    def extract(self, feats, utt_row_offsets, out=None, state=None, return_state=False):
        """OnlineIvectorFeature::GetFrame for every frame: `feats` = device [sum T x base_dim] base
        features of the utterances row-concatenated -> device [sum T x ivector_dim].  state: [n_utts x
        state_dim()] adaptation states the utterances start from (SetAdaptationState); return_state:
        also the states after them, before LimitFrames (GetAdaptationState)."""
        off = np.ascontiguousarray(utt_row_offsets, np.int32)
        if feats.shape[1] != self.cfg.base_dim or off[-1] != feats.shape[0]:
            raise KhError("OnlineIvectorFeature: feature dimension / row offsets mismatch")
        if out is None:
            out = torch.empty((feats.shape[0], self.cfg.ivector_dim), dtype=torch.float32, device=feats.device)
        n = len(off) - 1
        if state is None and not return_state:
            check(lib().kh_ivector_extract(self._h, _p(feats), _dim(feats).stride, off.ctypes.data_as(capi.c_int32_p), n,
                                           _p(out), _dim(out).stride))
            return out
        sin = None
        if state is not None:
            sin = np.ascontiguousarray(state, np.float64)
            if sin.shape != (n, self.state_dim()):
                raise KhError("OnlineIvectorFeature::SetAdaptationState: state of the wrong shape")
        sout = np.empty((n, self.state_dim())) if return_state else None
        dp = capi.c_double_p
        check(lib().kh_ivector_extract_adapt(self._h, _p(feats), _dim(feats).stride, off.ctypes.data_as(capi.c_int32_p), n,
                                             sin.ctypes.data_as(dp) if sin is not None else None,
                                             sout.ctypes.data_as(dp) if sout is not None else None, _p(out), _dim(out).stride))
        return (out, sout) if return_state else out

    def __del__(self):
        if getattr(self, "_h", None):
            capi.load().kh_ivector_extractor_destroy(self._h)
            self._h = None


class OnlineIvectorStreams:
    """OnlineIvectorFeature objects of n utterances side by side WITH frame weights (online-ivector-feature.h:299-362):
    the feature side of the silence weighting.  feats: device [sum T x base_dim]; state: [n x state_dim] adaptation
    states (None = fresh); out: device [sum T x ivector_dim] (may be a column block of a wider feature matrix) whose rows
    get_frames() fills."""

    def __init__(self, extractor, feats, utt_row_offsets, out, state=None):
        self.extractor = extractor
        self.off = np.ascontiguousarray(utt_row_offsets, np.int32)
        if feats.shape[1] != extractor.cfg.base_dim or self.off[-1] != feats.shape[0] or out.shape != (feats.shape[0], extractor.cfg.ivector_dim):
            raise KhError("OnlineIvectorFeature: feature dimension / row offsets mismatch")
        self.n = len(self.off) - 1
        st = None if state is None else np.ascontiguousarray(state, np.float64)
        if st is not None and st.shape != (self.n, extractor.state_dim()):
            raise KhError("OnlineIvectorFeature: one adaptation state per utterance")
        self._keep = (feats, out)
        h = lib().kh_ivector_streams_create(extractor._h, _p(feats), _dim(feats).stride, self.off.ctypes.data_as(capi.c_int32_p), self.n,
                                            st.ctypes.data_as(capi.c_double_p) if st is not None else None, _p(out), _dim(out).stride)
        if not h:
            raise KhError(lib().kh_last_error().decode())
        self._h = C.c_void_p(h)

    def __del__(self):
        try:
            if self._h:
                lib().kh_ivector_streams_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def update_frame_weights(self, stream, delta_weights, num_frames_ready):
        """UpdateFrameWeights(delta_weights) :155-170; delta_weights = [(frame, delta), ...]."""
        fr = np.ascontiguousarray([d[0] for d in delta_weights], np.int32)
        w = np.ascontiguousarray([d[1] for d in delta_weights], np.float32)
        check(lib().kh_ivector_streams_update_frame_weights(self._h, int(stream), len(fr), fr.ctypes.data_as(capi.c_int32_p),
                                                            w.ctypes.data_as(capi.c_float_p), int(num_frames_ready)))

    def get_frames(self, streams, until_frames):
        """GetFrame(until) for every listed stream: the statistics advance to that frame, the iVector rows up to it are valid."""
        s = np.ascontiguousarray(streams, np.int32)
        u = np.ascontiguousarray(until_frames, np.int32)
        if len(s):
            check(lib().kh_ivector_streams_get_frames(self._h, len(s), s.ctypes.data_as(capi.c_int32_p), u.ctypes.data_as(capi.c_int32_p)))

    def get_stats(self, states):
        """Writes the OnlineIvectorEstimationStats part of GetAdaptationState() into states [n x state_dim] (CMVN part untouched)."""
        st = np.ascontiguousarray(states, np.float64)
        assert st.shape == (self.n, self.extractor.state_dim())
        check(lib().kh_ivector_streams_get_stats(self._h, st.ctypes.data_as(capi.c_double_p)))
        return st


class OnlineNnet2FeaturePipeline:
    """online2/online-nnet2-feature-pipeline.{h,cc} for a batch of whole utterances (what
    online2-wav-nnet2-latgen-faster --online=false feeds the decoder): base features (OnlineMfcc,
    :83) of every waveform, the iVector of every frame (OnlineIvectorFeature, :105-106) and
    OnlineAppendFeature (:107-108): row = [mfcc, ivector]."""

    def __init__(self, mfcc, ivector_extractor=None):
        self.mfcc, self.ivector = mfcc, ivector_extractor
        if ivector_extractor is not None and ivector_extractor.cfg.base_dim != mfcc.num_ceps:
            raise KhError("OnlineNnet2FeaturePipeline: iVector extractor expects %d-dim base features, MFCC gives %d"
                          % (ivector_extractor.cfg.base_dim, mfcc.num_ceps))

    def dim(self):
        return self.mfcc.num_ceps + (self.ivector.ivector_dim if self.ivector is not None else 0)

    def compute(self, waves, speakers=None, max_remembered_frames=1000.0):
        """waves: list of 1-D float32 device tensors.  Returns (features [sum T x Dim()] on the device,
        utterance row offsets); an utterance shorter than one frame contributes no rows.  speakers: one
        label per waveform — the utterances of a speaker are processed in list order with the adaptation
        state carried from one to the next (SetAdaptationState / GetAdaptationState,
        online2-wav-nnet2-latgen-faster.cc:186-200, :283), round by round over the speakers."""
        base = [self.mfcc.compute(w) for w in waves]
        lens = np.array([b.shape[0] for b in base], np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        rows = int(off[-1])
        d0 = self.mfcc.num_ceps
        stride = (self.dim() + 3) // 4 * 4
        dev = waves[0].device if waves else "cuda"
        out = torch.empty((max(rows, 1), stride), dtype=torch.float32, device=dev)[:rows, :self.dim()]
        if rows == 0:
            return out, off
        for u, b in enumerate(base):
            if b.shape[0]:
                out[off[u]:off[u + 1], :d0] = b
        if self.ivector is None:
            return out, off
        if speakers is None:
            speakers = list(range(len(waves)))
        # round r: the r-th utterance (with frames) of every speaker, from the state its predecessor left
        queues = {}
        for u, s in enumerate(speakers):
            if lens[u] > 0:
                queues.setdefault(s, []).append(u)
        state = {s: self.ivector.fresh_state(1)[0] for s in queues}
        chained = any(len(q) > 1 for q in queues.values())
        r = 0
        while True:
            batch = [(s, q[r]) for s, q in queues.items() if r < len(q)]
            if not batch:
                break
            feats = torch.cat([base[u] for _, u in batch], 0).contiguous()
            boff = np.concatenate([[0], np.cumsum([lens[u] for _, u in batch])]).astype(np.int32)
            if chained:
                iv, st = self.ivector.extract(feats, boff, state=np.stack([state[s] for s, _ in batch]), return_state=True)
                self.ivector.limit_frames(st, max_remembered_frames)
                for j, (s, _) in enumerate(batch):
                    state[s] = st[j]
            else:
                iv = self.ivector.extract(feats, boff)
            for j, (_, u) in enumerate(batch):
                out[off[u]:off[u + 1], d0:] = iv[boff[j]:boff[j + 1]]
            r += 1
        return out, off


# ---------------------------------------------------------------- fMLLR estimation (csrc/kh_fmllr.hip)
# gmm-est-fmllr, gmm-est-fmllr-gpost and gmm-post-to-gpost for a batch of speakers, in the library's four stages.  The frames
# of all utterances are stacked by rows; an entry list is CSR over those frames: dict(feo [T + 1] int64, pdf [E] int32,
# weight [E] float32, goff [E + 1] int64 = the running sum of the entries' pdf sizes).
def _host_pdf_offsets(am):
    return np.ascontiguousarray(am.pdf_offsets.cpu().numpy(), np.int32)


def _feat_args(feats):
    _dim(feats)
    T, D = int(feats.shape[0]), int(feats.shape[1])
    return T, D, int(feats.stride(0)) if T > 1 else max(int(feats.stride(0)), D)


def fmllr_entries(pdf_posts, pdf_offsets):
    """The entry list of a Posterior over pdfs: a list over the stacked frames of [(pdf, weight), ...], each frame in the
    order given (convert_posterior_to_pdfs gives ascending pdfs)."""
    off = np.asarray(pdf_offsets, np.int64)
    feo = np.zeros(len(pdf_posts) + 1, np.int64)
    pdf, w = [], []
    for t, fr in enumerate(pdf_posts):
        for p, x in fr:
            pdf.append(int(p))
            w.append(x)
        feo[t + 1] = len(pdf)
    pdf = np.ascontiguousarray(pdf, np.int32)
    if len(pdf) and (pdf.min() < 0 or pdf.max() >= len(off) - 1):
        raise KhError("fmllr_entries: pdf %d, the model has %d" % (int(pdf.max() if pdf.min() >= 0 else pdf.min()), len(off) - 1))
    goff = np.zeros(len(pdf) + 1, np.int64)
    if len(pdf):
        goff[1:] = np.cumsum(off[pdf + 1] - off[pdf])
    return dict(feo=feo, pdf=pdf, weight=np.ascontiguousarray(w, np.float32), goff=goff)


def _entry_ptrs(ent, T):
    feo = np.ascontiguousarray(ent["feo"], np.int64)
    pdf = np.ascontiguousarray(ent["pdf"], np.int32)
    goff = np.ascontiguousarray(ent["goff"], np.int64)
    if len(feo) != T + 1 or len(goff) != len(pdf) + 1 or int(feo[-1]) != len(pdf):
        raise KhError("fmllr: entry list of %d frames / %d entries against %d frames" % (len(feo) - 1, len(pdf), T))
    return feo, pdf, goff


def gmm_component_posteriors(am, feats, ent):
    """DiagGmm::ComponentPosteriors (gmm/diag-gmm.cc:601-615) times the entry's weight, per entry (kh_gmm_component_posteriors).
    am: AmDiagGmm; feats: 2-D float32 device tensor.  Returns (gauss_post, like): device tensors of goff[E] and E floats."""
    return _component_posteriors(lib().kh_gmm_component_posteriors, am, feats, ent)


def _component_posteriors(entry, am, feats, ent):
    T, D, stride = _feat_args(feats)
    if D != am.dim:
        raise KhError("DiagGmm::ComponentLogLikelihood, dimension mismatch %d vs. %d" % (D, am.dim))
    feo, pdf, goff = _entry_ptrs(ent, T)
    w = np.ascontiguousarray(ent["weight"], np.float32)
    if len(w) != len(pdf):
        raise KhError("fmllr: %d weights for %d entries" % (len(w), len(pdf)))
    off = _host_pdf_offsets(am)
    post = torch.zeros(max(int(goff[-1]), 1), dtype=torch.float32, device=feats.device)
    like = torch.zeros(max(len(pdf), 1), dtype=torch.float32, device=feats.device)
    ip, lp = capi.c_int32_p, capi.c_int64_p
    check(entry(_p(feats), T, D, stride, _p(am.gconsts), _p(am.means_invvars), _p(am.inv_vars), off.ctypes.data_as(ip), am.num_pdfs,
                feo.ctypes.data_as(lp), pdf.ctypes.data_as(ip), w.ctypes.data_as(capi.c_float_p), goff.ctypes.data_as(lp), _p(post),
                _p(like)))
    return post[:int(goff[-1])], like[:len(pdf)]


def fmllr_frame_stats(am, feats, utt_row_offsets, spk_utt_offsets, ent, gauss_post):
    """FmllrDiagGmmAccs::AccumulateFromPosteriors per merged frame (kh_fmllr_frame_stats; the merging rule is stated in
    include/kaldi_hip.h).  am: the model whose means_invvars / inv_vars are accumulated.  Returns dict(run_row,
    spk_run_offsets [host], a, b [R x D float32 device], count [R float64 device])."""
    T, D, stride = _feat_args(feats)
    if D != am.dim:
        raise KhError("fmllr_frame_stats: feature dimension %d, model dimension %d" % (D, am.dim))
    feo, pdf, goff = _entry_ptrs(ent, T)
    uro = np.ascontiguousarray(np.asarray(utt_row_offsets, np.int32).reshape(-1))
    suo = np.ascontiguousarray(np.asarray(spk_utt_offsets, np.int32).reshape(-1))
    if gauss_post.numel() != int(goff[-1]) or gauss_post.dtype != torch.float32 or not gauss_post.is_cuda:
        raise KhError("fmllr_frame_stats: %d Gaussian posteriors for entries that hold %d" % (gauss_post.numel(), int(goff[-1])))
    gauss_post = gauss_post.contiguous()
    off = _host_pdf_offsets(am)
    n_spk = len(suo) - 1
    run_row, spk_run = np.zeros(T, np.int32), np.zeros(n_spk + 1, np.int32)
    a = torch.zeros((T, D), dtype=torch.float32, device=feats.device)
    b = torch.zeros((T, D), dtype=torch.float32, device=feats.device)
    count = torch.zeros(T, dtype=torch.float64, device=feats.device)
    ip, lp = capi.c_int32_p, capi.c_int64_p
    check(lib().kh_fmllr_frame_stats(_p(feats), T, D, stride, _p(am.means_invvars), _p(am.inv_vars), off.ctypes.data_as(ip),
                                     am.num_pdfs, uro.ctypes.data_as(ip), len(uro) - 1, suo.ctypes.data_as(ip), n_spk,
                                     feo.ctypes.data_as(lp), pdf.ctypes.data_as(ip), goff.ctypes.data_as(lp), _p(gauss_post),
                                     run_row.ctypes.data_as(ip), spk_run.ctypes.data_as(ip), _p(a), _p(b), _p(count)))
    R = int(spk_run[-1])
    return dict(run_row=run_row[:R].copy(), spk_run_offsets=spk_run, a=a[:R], b=b[:R], count=count[:R])


def fmllr_accumulate(feats, fs):
    """CommitSingleFrameStats over every speaker's merged frames (kh_fmllr_accumulate): dict(beta [S], K [S, D, D + 1],
    G [S, D, (D + 1)(D + 2) / 2]) float64 host arrays, G in SpMatrix packing."""
    T, D, stride = _feat_args(feats)
    run_row = np.ascontiguousarray(fs["run_row"], np.int32)
    spk_run = np.ascontiguousarray(fs["spk_run_offsets"], np.int32)
    S, R, P = len(spk_run) - 1, len(run_row), (D + 1) * (D + 2) // 2
    a, b, count = fs["a"].contiguous(), fs["b"].contiguous(), fs["count"].contiguous()
    if int(spk_run[-1]) != R or (R and (tuple(a.shape) != (R, D) or tuple(b.shape) != (R, D) or count.numel() != R)):
        raise KhError("fmllr_accumulate: %d merged frames, a %s, b %s, count %d" % (R, tuple(a.shape), tuple(b.shape), count.numel()))
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and count.dtype == torch.float64
    beta, K, G = np.zeros(S, np.float64), np.zeros((S, D, D + 1), np.float64), np.zeros((S, D, P), np.float64)
    ip, dp = capi.c_int32_p, capi.c_double_p
    check(lib().kh_fmllr_accumulate(_p(feats), T, D, stride, run_row.ctypes.data_as(ip), spk_run.ctypes.data_as(ip), S,
                                    _p(a) if R else None, _p(b) if R else None, _p(count) if R else None,
                                    beta.ctypes.data_as(dp), K.ctypes.data_as(dp), G.ctypes.data_as(dp)))
    return dict(beta=beta, K=K, G=G)


def fmllr_options(update_type="full", min_count=500.0, num_iters=40):
    """FmllrOptions (transform/fmllr-diag-gmm.h:43-56) with the reference's defaults."""
    return dict(update_type=update_type, min_count=float(min_count), num_iters=int(num_iters))


def fmllr_update(stats, update_type="full", min_count=500.0, num_iters=40, num_threads=0):
    """FmllrDiagGmmAccs::Update from a unit transform per speaker (kh_fmllr_update, host code).  Returns (transforms
    [S, D, D + 1] float32, objf_impr [S] float32, count [S] float32)."""
    beta = np.ascontiguousarray(stats["beta"], np.float64)
    K = np.ascontiguousarray(stats["K"], np.float64)
    G = np.ascontiguousarray(stats["G"], np.float64)
    S, D = K.shape[0], K.shape[1]
    if K.shape != (S, D, D + 1) or G.shape != (S, D, (D + 1) * (D + 2) // 2) or beta.shape != (S,):
        raise KhError("fmllr_update: stats of shapes %s %s %s" % (beta.shape, K.shape, G.shape))
    W, impr, count = np.zeros((S, D, D + 1), np.float32), np.zeros(S, np.float32), np.zeros(S, np.float32)
    dp, fp = capi.c_double_p, capi.c_float_p
    check(lib().kh_fmllr_update(S, D, beta.ctypes.data_as(dp), K.ctypes.data_as(dp), G.ctypes.data_as(dp), update_type.encode(),
                                float(min_count), int(num_iters), int(num_threads), W.ctypes.data_as(fp), impr.ctypes.data_as(fp),
                                count.ctypes.data_as(fp)))
    return W, impr, count


def fmllr_max_dim():
    return int(lib().kh_fmllr_max_dim())


def fmllr_frame_chunk():
    """Merged frames per workgroup of the accumulation kernel (kFrameChunk of csrc/kh_fmllr.hip)."""
    return int(lib().kh_fmllr_frame_chunk())


def fmllr_set_workspace_limit(nbytes):
    """fmllr_accumulate takes the speakers in groups whose workspace stays within nbytes (calling thread; 0 = 1 GiB)."""
    check(lib().kh_fmllr_set_workspace_limit(int(nbytes)))


def fmllr_last_timings():
    """Milliseconds of this thread's last calls of the four stages (whole calls, transfers and waits included)."""
    ms = (C.c_float * 6)()
    check(lib().kh_fmllr_last_timings(ms))
    return dict(component_posteriors_ms=ms[0], frame_stats_ms=ms[1], accumulate_ms=ms[2], update_ms=ms[3],
                accumulate_kernels_ms=ms[4], accumulate_groups=int(ms[5]))


def estimate_fmllr(am, feats, utt_row_offsets, spk_utt_offsets, posts=None, gposts=None, tid2pdf=None, opts=None, gpost_am=None,
                   return_stats=False):
    """gmm-est-fmllr (posts) or gmm-est-fmllr-gpost (gposts) for all speakers in one pass.  feats: the utterances' frames
    stacked, 2-D float32 device tensor; a speaker's utterances contiguous (spk_utt_offsets over utt_row_offsets).
    posts: a Posterior over the stacked frames, [(id, weight), ...] per frame, ids = transition-ids mapped through tid2pdf
    (None: they are pdf-ids already).  gposts: per frame [(pdf, posteriors array), ...] as gmm-post-to-gpost writes them; the
    statistics are then taken with gpost_am's means / variances when given (the two-model case), else am's.
    opts: fmllr_options().  Returns (transforms [S, D, D + 1], objf_impr [S], count [S]) (+ the statistics)."""
    if (posts is None) == (gposts is None):
        raise KhError("estimate_fmllr: give posts or gposts")
    opts = opts or fmllr_options()
    off = _host_pdf_offsets(am)
    if posts is not None:
        pdf_posts = convert_posterior_to_pdfs(tid2pdf, posts) if tid2pdf is not None else posts
        ent = fmllr_entries(pdf_posts, off)
        gauss_post, _ = gmm_component_posteriors(am, feats, ent)
        acc_am = am
    else:
        acc_am = gpost_am if gpost_am is not None else am
        sizes = np.diff(off.astype(np.int64))
        feo = np.zeros(len(gposts) + 1, np.int64)
        pdf, vecs = [], []
        for t, fr in enumerate(gposts):
            for p, v in fr:
                v = np.asarray(v, np.float32).reshape(-1)
                if not 0 <= int(p) < len(sizes) or len(v) != sizes[int(p)]:
                    raise KhError("estimate_fmllr: pdf %d has %s Gaussians, the gpost carries %d" %
                                  (int(p), sizes[int(p)] if 0 <= int(p) < len(sizes) else "no", len(v)))
                pdf.append(int(p))
                vecs.append(v)
            feo[t + 1] = len(pdf)
        goff = np.zeros(len(pdf) + 1, np.int64)
        if pdf:
            goff[1:] = np.cumsum([len(v) for v in vecs])
        ent = dict(feo=feo, pdf=np.ascontiguousarray(pdf, np.int32), weight=np.ones(len(pdf), np.float32), goff=goff)
        flat = np.concatenate(vecs) if vecs else np.zeros(0, np.float32)
        gauss_post = torch.as_tensor(flat, device=feats.device)
    fs = fmllr_frame_stats(acc_am, feats, utt_row_offsets, spk_utt_offsets, ent, gauss_post)
    stats = fmllr_accumulate(feats, fs)
    W, impr, count = fmllr_update(stats, opts["update_type"], opts["min_count"], opts["num_iters"])
    return (W, impr, count, stats) if return_stats else (W, impr, count)


def gmm_post_to_gpost(am, feats, pdf_posts):
    """gmm-post-to-gpost.cc:94-115 for the stacked frames: per frame [(pdf, posteriors), ...] without the vectors that are
    zero (IsZero's 1e-6 cutoff), and per entry (like, weight) for the tool's averages."""
    ent = fmllr_entries(pdf_posts, _host_pdf_offsets(am))
    post, like = gmm_component_posteriors(am, feats, ent)
    post, like = post.cpu().numpy(), like.cpu().numpy()
    out = []
    for t in range(len(pdf_posts)):
        fr = []
        for e in range(int(ent["feo"][t]), int(ent["feo"][t + 1])):
            v = post[int(ent["goff"][e]):int(ent["goff"][e + 1])]
            if np.abs(v).max() > 1.0e-06:                                                  # !this_post_vec.IsZero()
                fr.append((int(ent["pdf"][e]), v.copy()))
        out.append(fr)
    return out, like, ent["weight"]


# ---------------------------------------------------------------- GMM training statistics (csrc/kh_gmmacc.hip)
# The E-step of gmm-acc-stats-ali / gmm-acc-stats / gmm-acc-stats-twofeats for stacked frames, over the entry lists above.
kGmmMeans, kGmmVariances, kGmmWeights, kGmmTransitions, kGmmAll = 1, 2, 4, 8, 15


def gmm_flags(flags):
    """StringToGmmFlags then AugmentGmmFlags (gmm/model-common.cc:26-61), as AccumDiagGmm::Resize stores them and Write emits
    them: "mvwt" and kGmmAll -> 15 (the transition bit is kept: it is in the file), "mvw" and "v" -> 7, "m" -> 5, "" -> 4.  An
    int is taken as the reference's bits."""
    if isinstance(flags, str):
        bits = 0
        for c in flags:
            if c not in "mvwta":
                raise KhError("Invalid element '%s' of GmmFlagsType option string %s" % (c, flags))
            bits |= {"m": kGmmMeans, "v": kGmmVariances, "w": kGmmWeights, "t": kGmmTransitions, "a": kGmmAll}[c]
    else:
        bits = int(flags)
        if bits & ~kGmmAll:
            raise KhError("AugmentGmmFlags: (flags & ~kGmmAll) == 0, got %d" % bits)
    if bits & kGmmVariances:
        bits |= kGmmMeans
    return bits | kGmmWeights             # m needs w; and w is added to empty flags (with a warning in the reference)


def gmm_flags_to_string(bits):
    return "".join(c for c, b in (("m", 1), ("v", 2), ("w", 4), ("t", 8)) if bits & b)


def gmm_acc_component_posteriors(am, feats, ent):
    """gmm_component_posteriors with exp and log as the float of the double function (kh_gmm_acc_component_posteriors): the
    posteriors of the accumulation route, whose sums are written to a file as floats."""
    return _component_posteriors(lib().kh_gmm_acc_component_posteriors, am, feats, ent)


def gmm_acc_stats(am, feats, ent, gauss_post, flags="mvw"):
    """AccumDiagGmm::AccumulateFromPosteriors for every entry (kh_gmm_acc_stats).  am: AmDiagGmm (its pdf sizes are what is
    used); feats: the 2-D float32 device tensor the statistics are taken from, of any dimension up to gmm_acc_max_dim();
    gauss_post: the entries' Gaussian posteriors, float32 device tensor (gmm_acc_component_posteriors' output).  Returns
    dict(occ [NG], mean_acc [NG, D], var_acc [NG, D]) float64 host arrays; an accumulator the flags exclude is None.  The
    library call takes the m | v | w bits; the transition bit means nothing to it."""
    bits = gmm_flags(flags)
    T, D, stride = _feat_args(feats)
    feo, pdf, goff = _entry_ptrs(ent, T)
    if gauss_post.dtype != torch.float32 or not gauss_post.is_cuda or gauss_post.numel() != int(goff[-1]):
        raise KhError("gmm_acc_stats: %d Gaussian posteriors for entries that hold %d" % (gauss_post.numel(), int(goff[-1])))
    gauss_post = gauss_post.contiguous()
    off = _host_pdf_offsets(am)
    NG = int(off[-1])
    occ = np.zeros(NG, np.float64)
    mean = np.zeros((NG, D), np.float64) if bits & kGmmMeans else None
    var = np.zeros((NG, D), np.float64) if bits & kGmmVariances else None
    ip, lp, dp = capi.c_int32_p, capi.c_int64_p, capi.c_double_p
    check(lib().kh_gmm_acc_stats(_p(feats), T, D, stride, off.ctypes.data_as(ip), am.num_pdfs, feo.ctypes.data_as(lp),
                                 pdf.ctypes.data_as(ip), goff.ctypes.data_as(lp), _p(gauss_post), bits & 7, occ.ctypes.data_as(dp),
                                 mean.ctypes.data_as(dp) if mean is not None else None,
                                 var.ctypes.data_as(dp) if var is not None else None))
    return dict(occ=occ, mean_acc=mean, var_acc=var)


def gmm_acc_chunk():
    """Entries per chunk of the accumulation kernel (kChunk of csrc/kh_gmmacc.hip)."""
    return int(lib().kh_gmm_acc_chunk())


def gmm_acc_max_dim():
    return int(lib().kh_gmm_acc_max_dim())


def gmm_acc_set_workspace_limit(nbytes):
    """gmm_acc_stats takes the pdfs in groups whose workspace stays within nbytes (calling thread; 0 = 1 GiB)."""
    check(lib().kh_gmm_acc_set_workspace_limit(int(nbytes)))


def gmm_acc_last_timings():
    """The calling thread's last gmm_acc_stats: milliseconds of the call, its host plan and its kernels, and of the last
    gmm_acc_component_posteriors; groups, chunks, workgroups."""
    return _timings(lib().kh_gmm_acc_last_timings, ("call_ms", "plan_ms", "kernels_ms", "component_posteriors_ms"),
                    ("groups", "chunks", "workgroups"))


def accumulate_gmm_stats(am, feats, pdf_posts=None, alignments=None, tid2pdf=None, stats_feats=None, flags="mvw", into=None,
                         return_entries=False):
    """gmm_acc_component_posteriors on feats, then gmm_acc_stats on stats_feats or feats:
    AccumAmDiagGmm::AccumulateForGmm (mle-am-diag-gmm.cc:69-79) for every (frame, pdf, weight) of the stacked frames, or
    AccumulateForGmmTwofeats (:81-97) when stats_feats is given: the posteriors from feats, the statistics from stats_feats
    (the same rows, any dimension).  pdf_posts: [(pdf, weight), ...] per frame; or alignments (a transition-id per frame) with
    tid2pdf, every weight 1.  total_like adds fl32(like * weight) and total_frames the weight, doubles in entry order (:76-77).
    into: a dict this function returned, added to in double (pdf_offsets, dim and flags must agree).  Returns
    dict(occ, mean_acc, var_acc, pdf_offsets, dim, flags, total_like, total_frames); flags are the augmented GmmFlagsType as the
    file holds it ("mvwt" and kGmmAll: 15).  return_entries: also the entry list and the entries' scores (host float32), for a
    caller's per-utterance figures: (accumulator, ent, like)."""
    if (pdf_posts is None) == (alignments is None):
        raise KhError("accumulate_gmm_stats: give pdf_posts or alignments")
    off = _host_pdf_offsets(am)
    if pdf_posts is None:
        if tid2pdf is None:
            raise KhError("accumulate_gmm_stats: alignments need tid2pdf")
        pdf_posts = [[(int(tid2pdf[int(t)]), 1.0)] for t in alignments]
    bits = gmm_flags(flags)
    x2 = feats if stats_feats is None else stats_feats
    if int(x2.shape[0]) != int(feats.shape[0]):
        raise KhError("Features have mismatched numbers of frames %d vs. %d" % (feats.shape[0], x2.shape[0]))
    ent = fmllr_entries(pdf_posts, off)
    if len(ent["pdf"]):
        post, like = gmm_acc_component_posteriors(am, feats, ent)
        like = like.cpu().numpy()
    else:
        post, like = torch.zeros(0, dtype=torch.float32, device=feats.device), np.zeros(0, np.float32)
    acc = gmm_acc_stats(am, x2, ent, post, bits)
    # np.cumsum adds in order: the doubles of fl32(like * weight) and of the weights, entry by entry
    tot_like = float(np.cumsum((like * ent["weight"]).astype(np.float64))[-1]) if len(like) else 0.0
    tot_frames = float(np.cumsum(ent["weight"].astype(np.float64))[-1]) if len(like) else 0.0
    acc.update(pdf_offsets=off, dim=int(x2.shape[1]), flags=bits, total_like=tot_like, total_frames=tot_frames)
    acc = acc if into is None else add_gmm_stats(into, acc)
    return (acc, ent, like) if return_entries else acc


def add_gmm_stats(into, acc):
    """into += acc in double, with the checks (and messages) of AccumAmDiagGmm::Read / AccumDiagGmm::Read with add = true."""
    from . import kaldi_io
    try:
        return kaldi_io.add_gmm_accs(into, acc)
    except ValueError as e:
        raise KhError(str(e))


# ---------------------------------------------------------------- Gaussian selection, global GMM statistics (csrc/kh_gselect.hip)
# gmm-gselect and gmm-global-acc-stats for stacked frames and one DiagGmm: an AmDiagGmm of ONE pdf (diag_gmm makes it).
def diag_gmm(weights, means_invvars, inv_vars, device="cuda"):
    """A DiagGmm (kaldi_io.read_diag_gmm's arrays) on the device, gconsts computed as DiagGmm::Read does: an AmDiagGmm of one pdf."""
    g, _ = gmm_compute_gconsts(weights, means_invvars, inv_vars)
    return AmDiagGmm(g, means_invvars, inv_vars, np.asarray([0, len(g)], np.int32), device=device)


def _one_gmm(gmm, feats, what):
    if gmm.num_pdfs != 1:
        raise KhError("%s: a single DiagGmm is needed, the model has %d pdfs" % (what, gmm.num_pdfs))
    T, D, stride = _feat_args(feats)
    if D != gmm.dim:
        raise KhError("DiagGmm::ComponentLogLikelihood, dimension mismatch %d vs. %d" % (D, gmm.dim))
    return T, D, stride


def _csr_lists(lists, T, what):
    """A list per frame -> (offsets int64 [T + 1], items int32)."""
    if len(lists) != T:
        raise KhError("%s: %d lists for %d frames" % (what, len(lists), T))
    off = np.zeros(T + 1, np.int64)
    if T:
        off[1:] = np.cumsum([len(v) for v in lists])
    items = np.concatenate([np.asarray(v, np.int32).reshape(-1) for v in lists]).astype(np.int32) if int(off[-1]) else np.zeros(1, np.int32)
    return off, np.ascontiguousarray(items)


def gmm_gselect(gmm, feats, n, preselect=None):
    """DiagGmm::GaussianSelection for every stacked frame (kh_gmm_gselect), or GaussianSelectionPreselect when preselect (a
    list of Gaussians per frame) is given.  gmm: an AmDiagGmm of one pdf; feats: 2-D float32 device tensor.  Returns
    dict(lists: per frame an int32 array, best first; frame_like float32 [T]; status int32 [T], 1 for a frame with a NaN score,
    which has no selection).  The order, the scores and frame_like are stated in include/kaldi_hip.h."""
    T, D, stride = _one_gmm(gmm, feats, "gmm_gselect")
    G, n = gmm.num_mix, int(n)
    n_out = max(1, min(n, G))
    dev = feats.device
    sel = torch.empty((max(T, 1), n_out), dtype=torch.int32, device=dev)
    cnt = torch.empty(max(T, 1), dtype=torch.int32, device=dev)
    like = torch.empty(max(T, 1), dtype=torch.float32, device=dev)
    status = torch.empty(max(T, 1), dtype=torch.int32, device=dev)
    po = pg = None
    if preselect is not None:
        off, items = _csr_lists(preselect, T, "gmm_gselect")
        po, pg = off.ctypes.data_as(capi.c_int64_p), items.ctypes.data_as(capi.c_int32_p)
    check(lib().kh_gmm_gselect(_p(feats), T, D, stride, _p(gmm.gconsts), _p(gmm.means_invvars), _p(gmm.inv_vars), G, n, po, pg,
                               _p(sel), _p(cnt), _p(like), _p(status)))
    sel, cnt = sel[:T].cpu().numpy(), cnt[:T].cpu().numpy()
    return dict(lists=[sel[t, :cnt[t]].copy() for t in range(T)], frame_like=like[:T].cpu().numpy(), status=status[:T].cpu().numpy())


def gmm_preselect_posteriors(gmm, feats, gselect, weights=None):
    """The gselect branch of gmm-global-acc-stats.cc:117-131 up to the accumulation (kh_gmm_preselect_posteriors): per frame
    whose weight is not 0, LogLikelihoodsPreselect, ApplySoftMax in list order, Scale(weight).  gselect: a list of Gaussians per
    frame; weights: per frame, or None.  Returns (post, frame_like, used): post a float32 device tensor [used frames x
    num_gauss], dense and zero outside the lists; frame_like float32 host [T], 0 for a skipped frame; used: the frames that
    were not skipped, host int32.  A list that is empty or names a Gaussian twice on a used frame raises, naming the frame."""
    T, D, stride = _one_gmm(gmm, feats, "gmm_preselect_posteriors")
    off, items = _csr_lists(gselect, T, "gmm_preselect_posteriors")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        if len(w) != T:
            raise KhError("gmm_preselect_posteriors: %d weights for %d frames" % (len(w), T))
    used = np.arange(T, dtype=np.int32) if w is None else np.nonzero(w != 0)[0].astype(np.int32)
    G = gmm.num_mix
    post = torch.empty((max(len(used), 1), G), dtype=torch.float32, device=feats.device)
    like = torch.empty(max(T, 1), dtype=torch.float32, device=feats.device)
    check(lib().kh_gmm_preselect_posteriors(_p(feats), T, D, stride, _p(gmm.gconsts), _p(gmm.means_invvars), _p(gmm.inv_vars), G,
                                            off.ctypes.data_as(capi.c_int64_p), items.ctypes.data_as(capi.c_int32_p),
                                            w.ctypes.data_as(capi.c_float_p) if w is not None else None, _p(post), _p(like)))
    return post[:len(used)], like[:T].cpu().numpy(), used


def _used_entries(used, T, G):
    """The entry list kh_gmm_acc_stats takes for a one-pdf model: one entry per used frame."""
    feo = np.zeros(T + 1, np.int64)
    feo[np.asarray(used, np.int64) + 1] = 1
    feo = np.cumsum(feo)
    n = len(used)
    return dict(feo=feo, pdf=np.zeros(n, np.int32), weight=np.ones(n, np.float32), goff=np.arange(n + 1, dtype=np.int64) * G)


def accumulate_global_gmm_stats(gmm, feats, gselect=None, weights=None, flags="mvw", into=None):
    """The frame loop of gmm-global-acc-stats.cc:117-139 for the stacked frames of ONE utterance or batch.  With gselect:
    gmm_preselect_posteriors, then gmm_acc_stats unchanged on the dense posteriors (a zero posterior adds +-0 to a double sum,
    so the sums are those over the selected items).  Without: AccumulateFromDiag - gmm_acc_component_posteriors on the one-pdf
    model with the frame weights as entry weights, then gmm_acc_stats.  A frame of weight 0 is skipped.  Returns dict(occ,
    mean_acc, var_acc, dim, flags, file_like, file_weight): file_like is the reference's FLOAT running sum file_like += weight
    * like in frame order, file_weight the float sum of the weights, both made on the host.  into: a dict this function
    returned, whose occ / mean_acc / var_acc are added to in double (file_like / file_weight are this call's)."""
    T, D, stride = _one_gmm(gmm, feats, "accumulate_global_gmm_stats")
    G = gmm.num_mix
    bits = gmm_flags(flags)
    w = np.ones(T, np.float32) if weights is None else np.ascontiguousarray(weights, np.float32).reshape(-1)
    if len(w) != T:
        raise KhError("accumulate_global_gmm_stats: %d weights for %d frames" % (len(w), T))
    if gselect is not None:
        post, like, used = gmm_preselect_posteriors(gmm, feats, gselect, None if weights is None else w)
        ent = _used_entries(used, T, G)
        post = post.reshape(-1)
    else:
        used = np.nonzero(w != 0)[0].astype(np.int32)
        ent = _used_entries(used, T, G)
        ent["weight"] = w[used]
        like = np.zeros(T, np.float32)
        if len(used):
            post, el = gmm_acc_component_posteriors(gmm, feats, ent)
            like[used] = el.cpu().numpy()
        else:
            post = torch.zeros(0, dtype=torch.float32, device=feats.device)
    acc = gmm_acc_stats(gmm, feats, ent, post, bits) if T else dict(
        occ=np.zeros(G), mean_acc=np.zeros((G, D)) if bits & kGmmMeans else None, var_acc=np.zeros((G, D)) if bits & kGmmVariances else None)
    file_like, file_weight = np.float32(0.0), np.float32(0.0)
    for t in used:
        file_weight = np.float32(file_weight + w[t])
        file_like = np.float32(file_like + np.float32(w[t] * like[t]))
    acc.update(dim=D, flags=bits, file_like=file_like, file_weight=file_weight, frame_like=like)
    if into is not None:
        from . import kaldi_io
        try:
            kaldi_io.add_global_gmm_accs(into, acc)
        except ValueError as e:
            raise KhError(str(e))
        into.update(file_like=file_like, file_weight=file_weight, frame_like=like)
        return into
    return acc


def gselect_max_gauss():
    return int(lib().kh_gselect_max_gauss())


def gselect_max_n():
    return int(lib().kh_gselect_max_n())


def gselect_set_workspace_limit(nbytes):
    """gmm_gselect without a preselection scores at most nbytes of frames x Gaussians floats at a time (calling thread;
    0 = 256 MiB).  No result depends on it."""
    check(lib().kh_gselect_set_workspace_limit(int(nbytes)))


def gselect_last_timings():
    """The calling thread's last gmm_gselect (call, score kernels, selection kernels) and gmm_preselect_posteriors (call,
    kernel) in milliseconds; row chunks of the former, used frames of the latter."""
    return _timings(lib().kh_gselect_last_timings,
                    ("gselect_call_ms", "score_kernels_ms", "select_kernels_ms", "posteriors_call_ms", "posteriors_kernel_ms"),
                    ("row_chunks", "used_frames"))


# ---------------------------------------------------------------- MLLT statistics (csrc/kh_mllt.hip)
# gmm-acc-mllt for stacked frames, over the same entry lists.  An accumulator is dict(beta, G [D, D (D + 1) / 2] float64, dim):
# row j of G is the packed lower triangle of MlltAccs' G_[j].
def mllt_acc_stats(am, feats, ent, gauss_post):
    """MlltAccs::AccumulateFromPosteriors (transform/mllt.cc:131-160) for every entry, for Gaussian posteriors that RandPrune
    has already been applied to (kh_mllt_acc_stats).  am: AmDiagGmm; feats: 2-D float32 device tensor of the model's
    dimension, at most mllt_max_dim(); gauss_post: float32 device tensor.  Returns G, float64 host array [D, D (D + 1) / 2]."""
    T, D, stride = _feat_args(feats)
    if D != am.dim:
        raise KhError("MlltAccs::AccumulateFromPosteriors, dimension mismatch %d vs. %d" % (D, am.dim))
    feo, pdf, goff = _entry_ptrs(ent, T)
    if gauss_post.dtype != torch.float32 or not gauss_post.is_cuda or gauss_post.numel() != int(goff[-1]):
        raise KhError("mllt_acc_stats: %d Gaussian posteriors for entries that hold %d" % (gauss_post.numel(), int(goff[-1])))
    gauss_post = gauss_post.contiguous()
    off = _host_pdf_offsets(am)
    G = np.zeros((D, D * (D + 1) // 2), np.float64)
    ip, lp = capi.c_int32_p, capi.c_int64_p
    check(lib().kh_mllt_acc_stats(_p(feats), T, D, stride, _p(am.means_invvars), _p(am.inv_vars), off.ctypes.data_as(ip), am.num_pdfs,
                                  feo.ctypes.data_as(lp), pdf.ctypes.data_as(ip), goff.ctypes.data_as(lp), _p(gauss_post),
                                  G.ctypes.data_as(capi.c_double_p)))
    return G


def rand_prune(post, thresh, seed=None):
    """RandPrune (base/kaldi-math.h:169-175) on a host float32 array, in place and in order, with the C library's rand()
    (kh_rand_prune; no device).  seed: srand(seed) first; None leaves the generator as it is - a process that never seeds
    draws the reference's sequence.  Returns post."""
    if not isinstance(post, np.ndarray) or post.dtype != np.float32 or not post.flags.c_contiguous:
        raise KhError("rand_prune: a contiguous float32 host array is needed")
    check(lib().kh_rand_prune(post.ctypes.data_as(capi.c_float_p), post.size, float(thresh), 0 if seed is None else 1,
                              0 if seed is None else int(seed)))
    return post


def rand_prune_at(post, thresh, seed, skip):
    """rand_prune with the generator put in its place first: srand(seed), `skip` draws discarded (kh_rand_prune_at).  A
    process that uses the GPU does not own the C library's generator - the HIP runtime reseeds it when it initialises and
    draws from it at some first uses - so a job pruned in several calls passes seed 1 (the state of a process that never
    seeded) and the draws of its earlier calls.  Returns the number of draws taken."""
    if not isinstance(post, np.ndarray) or post.dtype != np.float32 or not post.flags.c_contiguous:
        raise KhError("rand_prune_at: a contiguous float32 host array is needed")
    draws = C.c_int64(0)
    check(lib().kh_rand_prune_at(post.ctypes.data_as(capi.c_float_p), post.size, float(thresh), int(seed), int(skip), C.byref(draws)))
    return int(draws.value)


_rand_prune = rand_prune       # accumulate_mllt_stats takes the reference's option name as a parameter


def mllt_chunk():
    """Items per slice of the MLLT accumulation, times a whole number (kChunk of csrc/kh_mllt.hip)."""
    return int(lib().kh_mllt_chunk())


def mllt_max_slices():
    return int(lib().kh_mllt_max_slices())


def mllt_max_dim():
    return int(lib().kh_mllt_max_dim())


def mllt_last_timings():
    """The calling thread's last mllt_acc_stats: milliseconds of the call, its host plan and its kernels; items, slices,
    workgroups."""
    return _timings(lib().kh_mllt_last_timings, ("call_ms", "plan_ms", "kernels_ms"), ("items", "slices", "workgroups"))


def _entry_sums(post, goff):
    """Per entry the double sum of its float posteriors in Gaussian order (this_beta_ of mllt.cc:143-157: a zero adds
    nothing), vectorised over the entries: one pass per Gaussian index."""
    goff = np.asarray(goff, np.int64)
    sizes = np.diff(goff)
    s = np.zeros(len(sizes), np.float64)
    for i in range(int(sizes.max()) if len(sizes) else 0):
        m = np.nonzero(sizes > i)[0]
        s[m] += post[goff[m] + i].astype(np.float64)
    return s


def accumulate_mllt_stats(am, feats, pdf_posts, rand_prune=0.25, seed=None, into=None, return_entries=False, segments=None):
    """MlltAccs::AccumulateFromGmm (mllt.cc:162-170) for every (frame, pdf, weight) of the stacked frames: the posteriors by
    gmm_acc_component_posteriors, brought to the host, pruned there in entry order then Gaussian order, beta as the double
    sum over the entries, in order, of each entry's double sum of its surviving posteriors, then the pruned posteriors back
    on the device and mllt_acc_stats.
    seed None: the pruning draws from the C library's generator as it stands (the module's rand_prune).  seed s: the job's
    draws are those of srand(s), and this call's begin where into's ended (rand_prune_at with into["draws"]): 1 gives what a
    reference binary draws, however the job is cut into calls and whatever else in the process touches the generator - the
    HIP runtime does.
    into: a dict this function returned (the dims must agree): G is added to it in double, and beta runs on from its beta
    entry by entry, as the reference's does from utterance to utterance.  Returns dict(beta, G, dim, draws), draws the
    job's so far.  return_entries: also the entry list and the entries' scores (host float32): (accumulator, ent, like).
    segments: row offsets [S + 1] of the call's utterances (0 ... T).  The posteriors, the pruning and the transfers are
    still one pass, but mllt_acc_stats then runs per segment and the segments' G are added in order, each into the running
    sum: a sum tree that depends on the utterances alone, so a job gives the same bits however its utterances are grouped
    into calls (the tool's --batch-frames).  Without segments the call is one accumulation, whose slices depend on where
    the call begins and ends."""
    thresh = rand_prune
    off = _host_pdf_offsets(am)
    ent = fmllr_entries(pdf_posts, off)
    before = 0 if into is None else int(into.get("draws", 0))
    draws = 0
    if len(ent["pdf"]):
        post, like = gmm_acc_component_posteriors(am, feats, ent)
        post, like = np.ascontiguousarray(post.cpu().numpy()), like.cpu().numpy()
        if seed is None:
            draws = int(((post != 0) & (np.abs(post) < np.float32(thresh))).sum())      # one draw for each such value
            _rand_prune(post, thresh)
        else:
            draws = rand_prune_at(post, thresh, seed, before)
        s = _entry_sums(post, ent["goff"])
        post = torch.from_numpy(post).to(feats.device)
    else:
        if float(thresh) < 0:
            raise KhError("rand_prune: prune threshold %g, must be >= 0" % thresh)
        post, like, s = torch.zeros(0, dtype=torch.float32, device=feats.device), np.zeros(0, np.float32), np.zeros(0)
    # beta_ += this_beta_, entry by entry, on from into's: however a job is cut into calls, beta is the same double
    beta = float(np.cumsum(np.concatenate([[0.0 if into is None else float(into["beta"])], s]))[-1])
    dim = int(feats.shape[1])
    acc = into if into is not None else dict(beta=0.0, G=np.zeros((dim, dim * (dim + 1) // 2), np.float64), dim=dim)
    if int(acc["dim"]) != dim:
        raise KhError("MlltAccs::Read, summing accs of different size.")         # as add_mllt_stats
    if segments is None:
        acc["G"] += mllt_acc_stats(am, feats, ent, post)
    else:
        seg = np.asarray(segments, np.int64).reshape(-1)
        if len(seg) < 1 or seg[0] != 0 or seg[-1] != feats.shape[0] or (np.diff(seg) < 0).any():
            raise KhError("accumulate_mllt_stats: segments must run from 0 to %d without going backwards" % feats.shape[0])
        feo, goff = ent["feo"], ent["goff"]
        for r0, r1 in zip(seg[:-1].tolist(), seg[1:].tolist()):
            e0, e1 = int(feo[r0]), int(feo[r1])
            if e1 > e0:
                g0, g1 = int(goff[e0]), int(goff[e1])
                sub = dict(feo=feo[r0:r1 + 1] - e0, pdf=ent["pdf"][e0:e1], weight=ent["weight"][e0:e1], goff=goff[e0:e1 + 1] - g0)
                acc["G"] += mllt_acc_stats(am, feats[r0:r1], sub, post[g0:g1])
    acc["beta"], acc["draws"] = beta, before + draws
    return (acc, ent, like) if return_entries else acc


def add_mllt_stats(into, acc):
    """into += acc in double, as MlltAccs::Read with add = true, with its size-mismatch message."""
    from . import kaldi_io
    try:
        return kaldi_io.add_mllt_accs(into, acc)
    except ValueError as e:
        raise KhError(str(e))


# ---------------------------------------------------------------- LDA statistics (csrc/kh_lda.hip)
# acc-lda for stacked frames.  An accumulator is dict(zero [C], first [C, D], second [D (D + 1) / 2] packed as SpMatrix packs,
# all float64; dim, num_classes); accumulate_lda_stats adds draws.  The entry list needs feo, pdf and weight only.
_LDA_MISMATCH = "LdaEstimate::Read, dimension or classes count mismatch, %d, %d,  vs. %d, %d"


def lda_acc_stats(feats, ent, num_classes, segments=None, into=None):
    """LdaEstimate::Accumulate (transform/lda-estimate.cc:45-55) for every entry whose weight is not zero, the weights being
    those RandPrune has already been applied to (kh_lda_acc_stats): one library call, whatever the number of segments.
    feats: 2-D float32 device tensor of at most lda_max_dim() columns; ent: dict(feo [T + 1], pdf [E], weight [E]);
    segments: row offsets [S + 1] of the call's utterances, from 0 to T (None: one segment).  into: an accumulator this
    function returned (dim and num_classes must agree): the library runs on from its buffers, segment after segment, so a
    job gives the same bits however its utterances are grouped into calls.  Returns dict(zero, first, second, dim,
    num_classes)."""
    T, D, stride = _feat_args(feats)
    C_ = int(num_classes)
    feo = np.ascontiguousarray(ent["feo"], np.int64)
    pdf = np.ascontiguousarray(ent["pdf"], np.int32)
    w = np.ascontiguousarray(ent["weight"], np.float32)
    if len(feo) != T + 1 or len(w) != len(pdf):
        raise KhError("lda_acc_stats: entry list of %d frames / %d entries / %d weights against %d frames" % (len(feo) - 1, len(pdf), len(w), T))
    if len(pdf) < int(feo.max()):
        raise KhError("lda_acc_stats: frame_entry_offsets reach %d, the list holds %d entries" % (int(feo.max()), len(pdf)))
    seg = np.ascontiguousarray([0, T] if segments is None else segments, np.int64).reshape(-1)
    if len(seg) < 1:
        raise KhError("lda_acc_stats: segments need at least one offset")
    if into is None:
        if C_ <= 0:
            raise KhError("lda_acc_stats: %d classes" % C_)
        acc = dict(zero=np.zeros(C_, np.float64), first=np.zeros((C_, D), np.float64), second=np.zeros(D * (D + 1) // 2, np.float64),
                   dim=D, num_classes=C_)
    else:
        acc = into
        if int(acc["dim"]) != D or int(acc["num_classes"]) != C_:
            raise KhError(_LDA_MISMATCH % (int(acc["num_classes"]), int(acc["dim"]), C_, D))
        for k, shape in (("zero", (C_,)), ("first", (C_, D)), ("second", (D * (D + 1) // 2,))):
            a = acc[k]
            if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != shape:
                raise KhError("lda_acc_stats: into[%r] must be a contiguous float64 array of shape %r" % (k, shape))
    dp, ip, lp = capi.c_double_p, capi.c_int32_p, capi.c_int64_p
    check(lib().kh_lda_acc_stats(_p(feats), T, D, stride, feo.ctypes.data_as(lp), pdf.ctypes.data_as(ip), w.ctypes.data_as(capi.c_float_p),
                                 C_, seg.ctypes.data_as(lp), len(seg) - 1, 0 if into is None else 1, acc["zero"].ctypes.data_as(dp),
                                 acc["first"].ctypes.data_as(dp), acc["second"].ctypes.data_as(dp)))
    return acc


def lda_chunk():
    """Items per slice of the LDA accumulation, times a whole number, and items per chunk of its first-order sums (kChunk of
    csrc/kh_lda.hip)."""
    return int(lib().kh_lda_chunk())


def lda_max_slices():
    return int(lib().kh_lda_max_slices())


def lda_max_dim():
    return int(lib().kh_lda_max_dim())


def lda_set_workspace_limit(nbytes):
    """lda_acc_stats takes the slices in passes whose workspace stays within nbytes (calling thread; 0 = 1 GiB)."""
    check(lib().kh_lda_set_workspace_limit(int(nbytes)))


def lda_last_timings():
    """The calling thread's last lda_acc_stats: milliseconds of the call, its host plan and its kernels; items, slices,
    workgroups, passes."""
    return _timings(lib().kh_lda_last_timings, ("call_ms", "plan_ms", "kernels_ms"), ("items", "slices", "workgroups", "passes"))


def lda_entries(pdf_posts):
    """The entry list of a Posterior over pdfs for lda_acc_stats: dict(feo, pdf, weight), each frame in the order given."""
    feo = np.zeros(len(pdf_posts) + 1, np.int64)
    pdf, w = [], []
    for t, fr in enumerate(pdf_posts):
        for p, x in fr:
            pdf.append(int(p))
            w.append(x)
        feo[t + 1] = len(pdf)
    return dict(feo=feo, pdf=np.ascontiguousarray(pdf, np.int32), weight=np.ascontiguousarray(w, np.float32))


def accumulate_lda_stats(feats, pdf_posts, num_pdfs, rand_prune=0.0, seed=None, into=None, segments=None):
    """The loop of bin/acc-lda.cc:99-110 for every (frame, pdf, weight) of the stacked frames: RandPrune on the weights on the
    host, strictly in utterance, frame, entry order, then lda_acc_stats - one library call.  pdf_posts: [(pdf, weight), ...]
    per frame (convert_posterior_to_pdfs: ascending pdfs).  rand_prune defaults to 0.0 as the binary's option does.
    seed None: the pruning draws from the C library's generator as it stands.  seed s: the job's draws are those of
    srand(s), and this call's begin where into's ended (rand_prune_at with into["draws"]): 1 gives what a reference binary
    draws, however the job is cut into calls.  into, segments: as lda_acc_stats.  Returns dict(zero, first, second, dim,
    num_classes, draws), draws the job's so far."""
    thresh = float(rand_prune)
    ent = lda_entries(pdf_posts)
    before = 0 if into is None else int(into.get("draws", 0))
    w = ent["weight"]
    if not thresh >= 0:
        raise KhError("rand_prune: prune threshold %g, must be >= 0" % thresh)
    if seed is None:
        draws = int(((w != 0) & (np.abs(w) < np.float32(thresh))).sum())      # one draw for each such value
        _rand_prune(w, thresh)
    else:
        draws = rand_prune_at(w, thresh, seed, before)
    acc = lda_acc_stats(feats, ent, num_pdfs, segments=segments, into=into)
    acc["draws"] = before + draws
    return acc


def add_lda_stats(into, acc):
    """into += acc in double, as LdaEstimate::Read with add = true, with its mismatch message."""
    from . import kaldi_io
    try:
        return kaldi_io.add_lda_accs(into, acc)
    except ValueError as e:
        raise KhError(str(e))


# ---------------------------------------------------------------- tree statistics (csrc/kh_tree.hip)
# acc-tree-stats for stacked frames.  An event (EventType) is a tuple of (key, value) pairs sorted by key: key -1 (kPdfClass)
# with the frame's pdf-class, key j with the phone at position j of the context window.
def tree_acc_stats(feats, frame_event, count, stats, add=True):
    """GaussClusterable::AddStats(row, 1.0) for every frame with an event (kh_tree_acc_stats): one library call.  feats: 2-D
    float32 device tensor of at most tree_max_dim() columns; frame_event [T] int32, -1 = frame not used; count [E] and stats
    [E, 2, D]: contiguous float64 host arrays, run on from (add) or overwritten.  Bit-equal to the reference's loop."""
    if feats.dim() == 2 and feats.shape[0] == 0 and feats.dtype == torch.float32 and feats.is_cuda:
        T, D, stride = 0, int(feats.shape[1]), int(feats.shape[1])            # no rows: the strides of an empty tensor say nothing
    else:
        T, D, stride = _feat_args(feats)
    fe = np.ascontiguousarray(frame_event, np.int32).reshape(-1)
    if len(fe) != T:
        raise KhError("tree_acc_stats: %d frame events against %d frames" % (len(fe), T))
    E = len(count)
    for name, a, shape in (("count", count, (E,)), ("stats", stats, (E, 2, D))):
        if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != shape:
            raise KhError("tree_acc_stats: %s must be a contiguous float64 array of shape %r" % (name, shape))
    dp = capi.c_double_p
    check(lib().kh_tree_acc_stats(_p(feats), T, D, stride, fe.ctypes.data_as(capi.c_int32_p), E, 1 if add else 0, count.ctypes.data_as(dp),
                                  stats.ctypes.data_as(dp)))


def tree_max_dim():
    return int(lib().kh_tree_max_dim())


def tree_tile():
    """Rows of an event's run staged per step (kTile of csrc/kh_tree.hip)."""
    return int(lib().kh_tree_tile())


def tree_last_timings():
    """The calling thread's last tree_acc_stats: milliseconds of the call, its host plan and its kernel; frames with an event,
    events with a frame, work items (waves), frames of the longest event."""
    return _timings(lib().kh_tree_last_timings, ("call_ms", "plan_ms", "kernels_ms"), ("frames", "events", "work_items", "longest"))


def tree_stats_ci_phones(text):
    """The --ci-phones string of acc-tree-stats (bin/acc-tree-stats.cc:80-87): colon-separated integers, sorted; a repeated
    phone or phone 0 is the binary's error."""
    if text == "":
        return []
    try:
        phones = sorted(int(w) for w in text.split(":"))
    except ValueError:
        raise KhError("Invalid set of ci_phones: " + text)
    if any(a == b for a, b in zip(phones, phones[1:])) or phones[0] == 0:
        raise KhError("Invalid set of ci_phones: " + text)
    return phones


def tree_stats_tables(tmodel):
    """What tree_stats_frame_events looks up per transition-id, beside read_transition_model's tables: the transition-state,
    the pdf-class of its HMM-state (TransitionIdToPdfClass), and per phone the pdf-class of the topology entry's state 0."""
    topo = tmodel["topo"]
    pdf_class = [-1]
    for phone, hmm_state, _ in np.asarray(tmodel["triples"]).reshape(-1, 3):
        entry = topo["entries"][topo["phone2idx"][int(phone)]]
        pdf_class += [int(entry[int(hmm_state)][0])] * len(entry[int(hmm_state)][1])
    first = np.full(len(topo["phone2idx"]), -1, np.int32)
    for ph in topo["phones"]:
        first[ph] = topo["entries"][topo["phone2idx"][ph]][0][0]
    return dict(tid2state=transition_id_to_state(tmodel), tid2pdf_class=np.asarray(pdf_class, np.int32), phone_first_pdf_class=first)


def _split_to_phones(tmodel, tables, ali):
    """SplitToPhones (hmm/hmm-utils.cc:594-701) on a non-empty alignment -> (was_ok, the phone instances' end points)."""
    n = len(ali)
    tstate, phone = tables["tid2state"][ali], tmodel["tid2phone"][ali]
    loop, final = tmodel["tid_is_self_loop"][ali], tmodel["tid_is_final"][ali]
    # IsReordered: the first change of transition-state with a self-loop on either side decides
    change = np.nonzero(tstate[:-1] != tstate[1:])[0]
    decided = change[loop[change] | loop[change + 1]]
    if len(decided):
        i = int(decided[0])
        if loop[i] and loop[i + 1]:
            raise KhError("KALDI_ASSERT: at IsReordered:hmm-utils.cc:602, failed: !(is_loop_1 && is_loop_2)")
        reordered = bool(loop[i])
    else:
        reordered = bool(not loop[0] and loop[-1])
    # SplitToPhonesInternal.  Reordered: the self-loops that follow a final transition-id belong to its phone and are stepped
    # over without being looked at.
    skipped = np.zeros(n, bool)
    if reordered:
        last_other = np.maximum.accumulate(np.where(~loop, np.arange(n), -1))      # the last position <= i that is no self-loop
        skipped = loop & (last_other >= 0) & final[np.maximum(last_other, 0)]
        bad = np.nonzero(skipped & (tstate != np.concatenate([[0], tstate[:-1]])))[0]
        if len(bad):
            raise KhError("KALDI_ASSERT: at SplitToPhonesInternal:hmm-utils.cc:645, failed: trans_model.TransitionIdToTransitionState("
                          "alignment[i]) == trans_model.TransitionIdToTransitionState(alignment[i+1])")
    nxt_state = np.concatenate([tstate[1:], [0]])
    nxt_phone = np.concatenate([phone[1:], [0]])
    last = np.arange(n) == n - 1
    error_end = ~final & (last | ((tstate != nxt_state) & (phone != nxt_phone)))   # an end the IsFinal check should have found
    looked_at = ~skipped
    is_end = looked_at & (final | error_end)
    was_ok = not bool((looked_at & error_end).any())
    # an end point is one past the position, or past the self-loops stepped over after it
    after = np.minimum.accumulate(np.where(looked_at, np.arange(n), n)[::-1])[::-1]   # the first looked-at position >= i
    after = np.concatenate([after[1:], [n]])
    ends = after[np.nonzero(is_end)[0]]
    starts = np.concatenate([[0], ends[:-1]])
    first_tid = ali[starts]
    emitting = tables["phone_first_pdf_class"][tmodel["tid2phone"][first_tid]] != -1
    if bool((emitting & (tmodel["tid2hmm_state"][first_tid] != 0)).any()):
        was_ok = False
    return was_ok, starts, ends


def tree_stats_frame_events(tmodel, alignment, N=3, P=1, ci_phones=(), phone_map=None, tables=None, codes=False):
    """The events of AccumulateTreeStats (hmm/tree-accu.cc:36-106) for one alignment -> (ok, events): ok False when
    SplitToPhones finds the alignment bad (the utterance then contributes nothing), else events[t] is the event of frame t.
    The alignment is cut into phone instances (SplitToPhones with IsReordered, hmm/hmm-utils.cc:594-701); an instance's event
    holds key j = 0 ... N - 1 with the phone at window position j around central position P - 0 outside the utterance, the
    phones through phone_map first - but only key P when the mapped central phone is one of ci_phones; each frame adds key -1
    (kPdfClass) with TransitionIdToPdfClass, and the pairs are sorted.  ci_phones: sorted and unique (tree_stats_ci_phones);
    phone_map: int array indexed by phone (kaldi_io.read_phone_map) or None; tables: tree_stats_tables(tmodel), made here
    when absent.  N and P of any sign are what the reference's loops make of them (a window that does not meet every phone
    instance once is its cur_pos assertion; N <= 0 keeps no phone key).  The work is per phone instance; a frame costs one
    list index.  codes=True -> (ok, table, code): the distinct (instance, pdf-class) events of the utterance and per frame
    its index into them (int32), events[t] = table[code[t]] - what TreeStats.accumulate(codes=...) takes without touching a
    tuple per frame.  Raises KhError with the reference's message where it asserts or errors."""
    ci = [int(p) for p in ci_phones]
    if any(a >= b for a, b in zip(ci, ci[1:])):
        raise KhError("KALDI_ASSERT: at AccumulateTreeStats:tree-accu.cc:46, failed: IsSortedAndUniq(ci_phones)")
    ali = np.asarray(alignment, np.int64).reshape(-1)
    if len(ali) == 0:
        return (True, [], np.zeros(0, np.int32)) if codes else (True, [])
    n_tids = len(tmodel["tid2pdf"]) - 1
    if ali.min() < 1 or ali.max() > n_tids:
        raise KhError("transition-id %d, the model has 1 .. %d" % (int(ali.max() if ali.min() >= 1 else ali.min()), n_tids))
    if tables is None:
        tables = tree_stats_tables(tmodel)
    ok, starts, ends = _split_to_phones(tmodel, tables, ali)
    if not ok:
        return (False, [], np.zeros(0, np.int32)) if codes else (False, [])
    L = len(starts)
    phones = tmodel["tid2phone"][ali[starts]].astype(np.int64)
    if phone_map is not None:                                 # MapPhone: 0 stays, out of range is the reference's error
        pm = np.asarray(phone_map, np.int64)
        out = np.nonzero((phones != 0) & ((phones < 0) | (phones >= len(pm))))[0]
        if len(out):
            raise KhError("Out-of-range phone %d bad --phone-map option?" % int(phones[out[0]]))
        phones = np.where(phones == 0, 0, pm[np.clip(phones, 0, len(pm) - 1)])
    # the windows i = -N ... L - 1 with their central instance i + P inside the utterance, in order: every instance must be
    # met exactly once (cur_pos runs through the alignment)
    centres = [i + P for i in range(-N, L) if 0 <= i + P < L]
    if centres != list(range(L)):
        raise KhError("KALDI_ASSERT: at AccumulateTreeStats:tree-accu.cc:105, failed: cur_pos == static_cast<int>(alignment.size())")
    padded = np.concatenate([np.zeros(max(N, 0) + abs(P), np.int64), phones, np.zeros(max(N, 0) + abs(P), np.int64)])
    base = max(N, 0) + abs(P) - P                             # instance c's window position j is padded[base + c + j]
    ci_set = set(ci)
    pdf_class = tables["tid2pdf_class"][ali]
    table, code = [], np.empty(len(ali), np.int64)
    for c in range(L):
        s, e = int(starts[c]), int(ends[c])
        window = padded[base + c:base + c + N].tolist()
        ctx_dep = int(phones[c]) not in ci_set
        context = tuple((j, window[j]) for j in range(N) if ctx_dep or j == P)
        classes, inverse = np.unique(pdf_class[s:e], return_inverse=True)
        code[s:e] = len(table) + inverse
        table += [tuple(sorted(context + ((-1, int(pc)),))) for pc in classes]
    if codes:
        return True, table, code.astype(np.int32)
    return True, [table[k] for k in code.tolist()]


class TreeStats:
    """The running statistics of acc-tree-stats: std::map<EventType, GaussClusterable*> as a host table of float64 rows that
    the library runs on from, batch after batch."""

    def __init__(self, dim, var_floor=0.01):
        self.dim = int(dim)
        self.var_floor = float(np.float32(var_floor))         # var_floor_ is a double that holds the float option
        self._row = {}
        self._count = np.zeros(0, np.float64)                 # the table's capacity: it doubles, len(self._row) rows are in use
        self._stats = np.zeros((0, 2, self.dim), np.float64)

    def __len__(self):
        return len(self._row)

    def accumulate(self, feats, frame_events, codes=None):
        """feats: 2-D float32 device tensor [T, dim]; frame_events: T events (tree_stats_frame_events), None for a frame
        that is not used.  With codes - int array [T], -1 for a frame that is not used - frame_events is instead a table of
        events (repeats allowed) and frame t has the event frame_events[codes[t]] (tree_stats_frame_events(codes=True), the
        utterances' tables joined): Python then works per table entry, not per frame.  The events the batch touches get
        local ids, their rows of the host table are gathered, ONE tree_acc_stats call runs on from them, and the rows are
        put back."""
        T = int(feats.shape[0])
        if int(feats.shape[1]) != self.dim:
            raise KhError("TreeStats.accumulate: features of dimension %d, the statistics have %d" % (int(feats.shape[1]), self.dim))
        local = {}
        if codes is None:
            if len(frame_events) != T:
                raise KhError("TreeStats.accumulate: %d frame events against %d frames" % (len(frame_events), T))
            fe = np.asarray([-1 if ev is None else local.setdefault(ev, len(local)) for ev in frame_events], np.int32)
        else:
            codes = np.asarray(codes, np.int64).reshape(-1)
            if len(codes) != T:
                raise KhError("TreeStats.accumulate: %d frame events against %d frames" % (len(codes), T))
            if len(codes) and (codes.min() < -1 or codes.max() >= len(frame_events)):
                raise KhError("TreeStats.accumulate: a code outside -1 ... %d" % (len(frame_events) - 1))
            met = np.unique(codes[codes >= 0])                # a table entry no frame names does not become an event
            of_entry = np.full(len(frame_events) + 1, -1, np.int32)          # [-1] serves the frames that are not used
            of_entry[met] = [local.setdefault(frame_events[k], len(local)) for k in met.tolist()]
            fe = of_entry[codes]
        new = [ev for ev in local if ev not in self._row]
        if new:
            need = len(self._row) + len(new)
            if need > len(self._count):
                room = max(need, 2 * len(self._count), 1024)
                self._count = np.concatenate([self._count, np.zeros(room - len(self._count), np.float64)])
                self._stats = np.concatenate([self._stats, np.zeros((room - len(self._stats), 2, self.dim), np.float64)])
            for ev in new:
                self._row[ev] = len(self._row)
        rows = np.asarray([self._row[ev] for ev in local], np.int64)
        count, stats = np.ascontiguousarray(self._count[rows]), np.ascontiguousarray(self._stats[rows])
        tree_acc_stats(feats, fe, count, stats, add=True)
        self._count[rows], self._stats[rows] = count, stats

    def items(self):
        """(event, dict(count, var_floor, stats [2, dim])) in std::map<EventType> order: the pairs compared in turn."""
        for ev in sorted(self._row):
            r = self._row[ev]
            yield ev, dict(count=float(self._count[r]), var_floor=self.var_floor, stats=self._stats[r])


# ---- host posterior / transform algebra of the fMLLR recipes
def weight_silence_post(tid2phone, silence_phones, silence_scale, post, distribute=False):
    """WeightSilencePost / WeightSilencePostDistributed (hmm/posterior.cc:361-413): tid2phone indexed by transition-id."""
    sil = set(int(p) for p in silence_phones)
    f32 = np.float32
    scale = f32(silence_scale)
    out = []
    for fr in post:
        if not distribute:
            this = []
            for tid, w in fr:
                if int(tid2phone[tid]) in sil:
                    if scale != 0.0:
                        this.append((tid, float(f32(f32(w) * scale))))
                else:
                    this.append((tid, float(f32(w))))
            out.append(this)
            continue
        sw, nw = f32(0.0), f32(0.0)
        for tid, w in fr:
            if int(tid2phone[tid]) in sil:
                sw = f32(sw + f32(w))
            else:
                nw = f32(nw + f32(w))
        if sw < 0.0 or nw < 0.0:
            raise KhError("KALDI_ASSERT: sil_weight >= 0.0 && nonsil_weight >= 0.0")
        if f32(sw + nw) == 0.0:
            out.append(list(fr))
            continue
        fscale = f32(f32(f32(sw * scale) + nw) / f32(sw + nw))
        out.append([(tid, float(f32(f32(w) * fscale))) for tid, w in fr] if fscale != 0.0 else [])
    return out


def compose_transforms(a, b, b_is_affine=False):
    """ComposeTransforms (transform/transform-common.cc:132-166) on host float32 matrices; None for an empty matrix."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if b.shape[0] == 0 or a.shape[1] == 0:
        return None
    if a.shape[1] == b.shape[0]:
        be = b
    elif a.shape[1] == b.shape[0] + 1:
        be = np.zeros((b.shape[0] + 1, b.shape[1] + (0 if b_is_affine else 1)), np.float32)
        be[:b.shape[0], :b.shape[1]] = b
        be[-1, -1] = 1.0
    else:
        raise KhError("ComposeTransforms: mismatched dimensions, a has %d columns and b has %d rows." % (a.shape[1], b.shape[0]))
    return (a.astype(np.float64) @ be.astype(np.float64)).astype(np.float32)


def transform_feats(trans, feats, out=None):
    """featbin/transform-feats.cc:98-118 on the device: linear when the transform has feature-dim columns, affine (an
    implicit 1.0 appended to the features) with one more; KhError otherwise.  trans, feats: 2-D float32 device tensors."""
    rows, cols, dim = int(trans.shape[0]), int(trans.shape[1]), int(feats.shape[1])
    if cols not in (dim, dim + 1):
        raise KhError("Transform matrix has bad dimension %dx%d versus feat dim %d%s" % (
            rows, cols, dim, " [perhaps the transform was created by compose-transforms, and you forgot the --b-is-affine option?]"
            if cols == dim + 2 else ""))
    if out is None:
        out = torch.empty((feats.shape[0], rows), dtype=torch.float32, device=feats.device)
    add_mat_mat(out, 1.0, feats, kNoTrans, trans[:, :dim], kTrans, 0.0)
    if cols == dim + 1:
        add_vec_to_rows(out, 1.0, trans[:, dim].contiguous())
    return out
