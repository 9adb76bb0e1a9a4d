"""GPU: kh_gmm_gselect (csrc/kh_gselect.hip) through api.gmm_gselect against the line-by-line restatement in library mode
(tests/gselect_restatement.py): lists, counts, status and frame_like bit for bit; without a preselection also against
kh_diag_gmm_loglikes' own output ordered by numpy.lexsort on (index, score).  Shapes: the wave width and the small / large
kernel forms' edges in G, n from 1 to the exported maximum, more frames than one workgroup holds, a row pitch above D, a row
chunk limit that cuts T unevenly; ties within a lane's column, across lanes, everywhere; preselections; the refusals before
any launch; a NaN row."""
import ctypes

import numpy as np
import pytest
import torch

import gselect_cases as GC
import gselect_restatement as R

pytestmark = pytest.mark.gpu


def check(api, m, x, wide, n, preselect=None, chunk_rows=None):
    gmm = GC.device_model(api, m)
    feats = GC.device_features(x, wide)
    G = len(m["gconsts"])
    if chunk_rows:
        api.gselect_set_workspace_limit(chunk_rows * G * 4)
    try:
        got = api.gmm_gselect(gmm, feats, n, preselect)
    finally:
        api.gselect_set_workspace_limit(0)
    if chunk_rows:
        assert api.gselect_last_timings()["row_chunks"] == -(-len(x) // chunk_rows)
    want_lists, want_like, want_status = R.gaussian_selection(m, x, n, preselect)
    assert np.array_equal(got["status"], want_status)
    assert [v.tolist() for v in got["lists"]] == want_lists
    assert np.array_equal(got["frame_like"].view(np.int32), want_like.view(np.int32))
    if preselect is None:
        ll = gmm.log_likelihoods(feats).cpu().numpy()
        for t in np.nonzero(want_status == 0)[0]:
            order = np.lexsort((np.arange(G), ll[t]))[::-1][:min(n, G)]      # score descending, then index descending
            assert got["lists"][t].tolist() == order.tolist(), t
    return got


MAXG, MAXN, SMALL = 4096, 128, 512

SHAPES = [  # G, n, D, T, stride
    (1, 1, 1, 1, None), (1, 4, 3, 5, None), (2, 1, 3, 5, None), (2, 2, 1, 5, 4), (63, 62, 3, 5, None), (63, 63, 40, 5, None),
    (64, 64, 40, 5, None), (64, 67, 3, 257, None), (65, 64, 1, 257, None), (65, 65, 3, 5, 8), (130, MAXN, 3, 5, None),
    (130, 1, 40, 257, 43), (130, 2, 3, 1, None), (SMALL, 30, 40, 257, None), (SMALL + 1, 5, 3, 5, None),
    (MAXG, MAXN, 3, 5, None), (MAXG, 65, 40, 1, None), (2048, 5, 40, 5, None),
]


def test_exported_limits(api):
    assert api.gselect_max_gauss() == MAXG and api.gselect_max_n() == MAXN
    assert api.lib().kh_gselect_small_lists() == SMALL and api.lib().kh_gselect_max_dim() == 96


@pytest.mark.parametrize("G,n,D,T,stride", SHAPES)
def test_shapes(api, G, n, D, T, stride):
    x, wide = GC.features(G + n, T, D, stride)
    check(api, GC.model(G * 7 + D, G, D), x, wide, n)


@pytest.mark.parametrize("rows", [1, 100, 256, 257, 1000])
def test_row_chunks_change_nothing(api, rows):
    m = GC.model(1, 70, 5)
    x, wide = GC.features(2, 257, 5)
    a = check(api, m, x, wide, 6, chunk_rows=rows)
    b = check(api, m, x, wide, 6)
    assert [v.tolist() for v in a["lists"]] == [v.tolist() for v in b["lists"]] and np.array_equal(a["frame_like"], b["frame_like"])


def test_chunks_on_both_sides_of_the_score_kernels_threshold(api):
    """kh_diag_gmm_loglikes takes its two-GEMM form from 2^22 scores per call: 1100 frames of 4096 Gaussians cut into chunks of
    1024 rows (the GEMM form) and 76 (the register form), and whole (the GEMM form) - the same lists and bits, the restatement's."""
    m = GC.model(5, MAXG, 3)
    x, wide = GC.features(6, 1100, 3)
    a = check(api, m, x, wide, 5, chunk_rows=1024)
    b = check(api, m, x, wide, 5)
    assert [v.tolist() for v in a["lists"]] == [v.tolist() for v in b["lists"]] and np.array_equal(a["frame_like"], b["frame_like"])


@pytest.mark.parametrize("same,G", [([(3, 67), (3, 131)], 140), ([(5, 6), (70, 71), (63, 64)], 140), ("all", 140), ("all", 600),
                                    ([(0, 1), (0, 64), (0, 65)], 66)], ids=["column", "lanes", "all-140", "all-600", "both"])
def test_ties(api, same, G):
    pairs = [(0, b) for b in range(1, G)] if same == "all" else same
    m = GC.model(11, G, 4, pairs)
    x, wide = GC.features(12, 7, 4)
    for n in (1, 2, 3, 64, 65, G):
        got = check(api, m, x, wide, min(n, MAXN))
        if same == "all":
            assert got["lists"][0].tolist() == list(range(G - 1, G - 1 - min(n, MAXN), -1))


@pytest.mark.parametrize("kind", ["contiguous", "scattered", "unsorted"])
@pytest.mark.parametrize("lengths,G", [([1], 70), ([64], 70), ([65], 70), ([1, 64, 65, 3, 70], 70), ([600, 2, 513], 700)],
                         ids=["1", "64", "65", "mixed", "large"])
def test_preselection(api, kind, lengths, G):
    m = GC.model(21, G, 6, [(2, 3), (2, 67)])
    x, wide = GC.features(22, 13, 6, 9)
    pre = GC.lists(23, 13, G, lengths, kind)
    for n in (1, 5, 64, 128):
        check(api, m, x, wide, n, pre)


def test_preselection_may_list_a_gaussian_twice(api):
    m = GC.model(31, 9, 3)
    x, wide = GC.features(32, 4, 3)
    pre = [[4, 4, 1], [0, 8, 0, 8], [7], [2, 3, 2]]
    got = check(api, m, x, wide, 3, pre)
    assert sorted(got["lists"][0].tolist()) == [1, 4, 4]


def _raw(api, m, T=3, D=None, stride=None, G=None, n=2, off=None, items=None):
    """kh_gmm_gselect itself -> (rc, message).  The outputs hold a canary: a refused call writes nothing."""
    gmm = GC.device_model(api, m)
    Dm = m["means_invvars"].shape[1]
    D = Dm if D is None else D
    feats = torch.zeros((T, max(D, 1)), dtype=torch.float32, device="cuda")
    sel = torch.full((T, 8), 77, dtype=torch.int32, device="cuda")
    cnt = torch.full((T,), 77, dtype=torch.int32, device="cuda")
    like = torch.full((T,), 77.0, dtype=torch.float32, device="cuda")
    st = torch.full((T,), 77, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    o = None if off is None else np.asarray(off, np.int64)
    it = None if items is None else np.asarray(items, np.int32)
    rc = api.lib().kh_gmm_gselect(p(feats), T, D, max(D, 1) if stride is None else stride, p(gmm.gconsts), p(gmm.means_invvars),
                                  p(gmm.inv_vars), gmm.num_mix if G is None else G, n,
                                  None if o is None else o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  None if it is None else it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), p(sel), p(cnt), p(like), p(st))
    torch.cuda.synchronize()
    if rc != 0:
        assert (sel == 77).all() and (cnt == 77).all() and (like == 77).all() and (st == 77).all()
    return rc, api.lib().kh_last_error().decode()


def test_refusals_before_any_launch(api):
    m = GC.model(41, 6, 3)
    fn = "kh_gmm_gselect: "
    assert _raw(api, m)[0] == 0
    assert _raw(api, m, G=MAXG + 1) == (-1, fn + "%d Gaussians, supported 1 ... %d" % (MAXG + 1, MAXG))
    assert _raw(api, m, G=0) == (-1, fn + "0 Gaussians, supported 1 ... %d" % MAXG)
    assert _raw(api, m, n=MAXN + 1) == (-1, fn + "num_gselect %d, supported 1 ... %d" % (MAXN + 1, MAXN))
    assert _raw(api, m, n=0) == (-1, fn + "num_gselect 0, supported 1 ... %d" % MAXN)
    assert _raw(api, m, n=-3) == (-1, fn + "num_gselect -3, supported 1 ... %d" % MAXN)
    assert _raw(api, m, D=97) == (-1, fn + "feature dimension 97, supported 1 ... 96")
    assert _raw(api, m, D=0) == (-1, fn + "feature dimension 0, supported 1 ... 96")
    assert _raw(api, m, stride=2) == (-1, fn + "feat_stride 2 is less than the feature dimension 3")
    ok = dict(off=[0, 1, 3, 4], items=[0, 5, 1, 2])
    assert _raw(api, m, **ok)[0] == 0
    assert _raw(api, m, off=[1, 1, 3, 4], items=[0, 5, 1, 2]) == (-1, fn + "pre_offsets[0] = 1, not 0")
    assert _raw(api, m, off=[0, 2, 1, 4], items=[0, 5, 1, 2]) == (-1, fn + "pre_offsets runs backwards at frame 1")
    assert _raw(api, m, off=[0, 1, 3, 4], items=[0, 5, 6, 2]) == (-1, fn + "frame 1 lists Gaussian 6, the model has 6")
    assert _raw(api, m, off=[0, 1, 3, 4], items=[0, 5, 1, -1]) == (-1, fn + "frame 2 lists Gaussian -1, the model has 6")
    assert _raw(api, m, off=[0, 1, 1, 2], items=[0, 5]) == (-1, fn + "frame 1 has an empty list")
    assert _raw(api, m, off=[0, 1, 8, 9], items=[0, 1, 1, 1, 1, 1, 1, 1, 2]) == (-1, fn + "frame 1 lists 7 Gaussians, at most 6")
    with pytest.raises(api.KhError, match="num_gselect 0"):
        api.gmm_gselect(GC.device_model(api, m), torch.zeros((2, 3), device="cuda"), 0)
    with pytest.raises(api.KhError, match="dimension mismatch 4 vs. 3"):
        api.gmm_gselect(GC.device_model(api, m), torch.zeros((2, 4), device="cuda"), 2)


def test_no_frames(api):
    got = api.gmm_gselect(GC.device_model(api, GC.model(51, 6, 3)), torch.zeros((0, 3), device="cuda"), 2)
    assert got["lists"] == [] and len(got["frame_like"]) == 0


@pytest.mark.parametrize("G", [70, 600])
def test_nan_row_sets_that_frames_status_only(api, G):
    m = GC.model(61, G, 3)
    x, wide = GC.features(62, 9, 3)
    x[4, 1] = np.nan
    got = check(api, m, x, wide, 5)
    assert got["status"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0] and len(got["lists"][4]) == 0 and np.isnan(got["frame_like"][4])
    pre = GC.lists(63, 9, G, [3, 66], "unsorted")
    got = check(api, m, x, wide, 5, pre)
    assert got["status"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]


def test_the_same_input_gives_the_same_bits(api):
    m = GC.model(71, 300, 10)
    x, wide = GC.features(72, 257, 10)
    gmm, feats = GC.device_model(api, m), GC.device_features(x, wide)
    a, b = api.gmm_gselect(gmm, feats, 20), api.gmm_gselect(gmm, feats, 20)
    assert [v.tolist() for v in a["lists"]] == [v.tolist() for v in b["lists"]]
    assert np.array_equal(a["frame_like"].view(np.int32), b["frame_like"].view(np.int32))
    t = api.gselect_last_timings()
    assert t["gselect_call_ms"] >= t["score_kernels_ms"] + t["select_kernels_ms"] > 0 and t["row_chunks"] == 1
