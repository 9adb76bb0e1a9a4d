"""Every kernel branch and tile edge of the GMM scoring (kh_gmm.hip): the five instantiations of the register
kernel and its second trip over the Gaussians, the two-GEMM path, both instantiations of the fused kernel on pdf-size
lists that put its tiles, chunk loops and boundary buffers on their edges, the split of the tile list, the fallback
for a pdf too large for a tile, both LogSumExp kernels at both of their boundaries, the second slab, pdfs whose
scores the test dictates bit for bit, and the contract of pdf_offsets.

Every test first asserts the restated launch decision (tests/gmm_cases.py) that puts the case into its branch, runs
on views into NaN-filled buffers with row padding, and afterwards requires the padding to be NaN still.  References:
the CPU oracle, bit-exact for the per-Gaussian scores, and for the per-pdf scores the float64 LogSumExp of those
scores with the bound derived in gmm_cases.py (test_gmm_reference.py checks both on the CPU); the project's 1e-4
against the oracle is asserted as well.  Where the oracle would take long it runs on a row subset: rows are
independent, and the subset holds the first and last row and both sides of every 64-frame and slab boundary."""
import importlib
import os

import numpy as np
import pytest

import cases
import dense_dispatch as dd
import gmm_cases as gc

pytestmark = pytest.mark.gpu
KhError = importlib.import_module("old-kaldi-git_amd.capi").KhError

PRUNES = (-1.0, 4.0, 0.5)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def device_model(api, g, mi, iv, off, param_offset=0):
    """AmDiagGmm on the device; param_offset = 1 puts means_invvars and inv_vars 4 bytes past a 16-byte boundary
    (dense rows, as the library requires: the fused kernel's 16-byte loads are then unaligned for every tile)."""
    gmm = api.AmDiagGmm(g, mi, iv, off)
    views = []
    if param_offset:
        views = [dd.mat(mi, 0, param_offset), dd.mat(iv, 0, param_offset)]
        gmm.means_invvars, gmm.inv_vars = views[0].t, views[1].t
        assert gmm.means_invvars.is_contiguous() and gmm.means_invvars.data_ptr() % 16 == 4 * param_offset
    return gmm, views


def pdf_scores(gmm, x, prune, pad=2, offset=1):
    out = dd.NanView(x.shape[0], gmm.num_pdfs, gmm.num_pdfs + pad, offset)
    gmm.pdf_log_likelihoods(x.t, log_sum_exp_prune=prune, out=out.t)
    got = out.host()
    out.assert_padding_untouched()
    return got


def gaussian_scores(gmm, x, pad=3, offset=1):
    out = dd.NanView(x.shape[0], gmm.num_mix, gmm.num_mix + pad, offset)
    gmm.log_likelihoods(x.t, out=out.t)
    got = out.host()
    out.assert_padding_untouched()
    return got


def frames_past_threshold(M, tmod):
    """The first T with T * M >= 1 << 22 and T mod 64 == tmod."""
    T = -(-gc.GEMM_THRESHOLD // M)
    return T + (tmod - T) % 64


def check_pdf_scores(api, oracle, monkeypatch, model, x_host, label, expect_fused, prunes=PRUNES, rows=None,
                     data_pad=1, data_offset=0, param_offset=0):
    """The per-pdf scores of one model on one set of frames, through the path kh_am_gmm_loglikes picks and through
    the unfused one: bit-identical; inside the derived bound against the float64 LogSumExp of the GPU's own
    per-Gaussian scores, which are bit-exact against the oracle on `rows`; inside 1e-4 of the oracle on `rows`."""
    off, g, mi, iv = model
    T, D = x_host.shape
    M, rows = len(g), np.arange(T) if rows is None else rows
    assert gc.fused_taken(T, D, M, off, os.environ) == expect_fused
    x = dd.mat(x_host, data_pad, data_offset)
    gmm, views = device_model(api, g, mi, iv, off, param_offset)
    ll = gaussian_scores(gmm, x)
    assert np.isfinite(ll).all()
    cases.exact(ll[rows], oracle.diag_gmm_loglikes_stored(x_host[rows], g, mi, iv))
    worst = 0.0
    for prune in prunes:
        got = pdf_scores(gmm, x, prune)
        with monkeypatch.context() as mp:
            mp.setenv("KH_GMM_NO_FUSION", "1")
            assert not gc.fused_taken(T, D, M, off, os.environ)
            plain = pdf_scores(gmm, x, prune, pad=1, offset=0)
        assert np.isfinite(got).all()
        assert same_bits(got, plain)
        ref, _ = gc.lse_reference(ll, off, prune)
        ratio = gc.bound_ratio(got, ref, off)
        worst = max(worst, ratio)
        assert ratio <= 1.0, "prune %g: error / bound = %.3f" % (prune, ratio)
        want = oracle.am_gmm_loglikes(x_host[rows], g, mi, iv, off, prune)
        assert np.abs(got[rows] - want).max() < 1e-4
    for v in [x] + views:
        v.assert_padding_untouched()
    print("gmm-ratio gpu %s %.3f" % (label, worst))
    return gmm, x


# ---------------------------------------------------------------- a. register kernel
REGISTER_CASES = [   # (DP, D, T, M): every D, T and M of the edges at least once, a few crossed per instantiation
    (16, 1, 1, 1), (16, 1, 64, 63), (16, 16, 65, 130), (16, 16, 257, 700),
    (32, 17, 63, 64), (32, 32, 257, 65), (32, 32, 1, 700),
    (40, 33, 64, 63), (40, 40, 65, 700), (40, 40, 257, 130),
    (64, 41, 63, 65), (64, 64, 257, 700), (64, 64, 64, 1),
    (96, 65, 65, 64), (96, 96, 257, 130), (96, 96, 63, 700), (96, 96, 1, 63),
]


@pytest.mark.parametrize("dp,D,T,M", REGISTER_CASES)
def test_register_kernel_every_instantiation(api, oracle, dp, D, T, M):
    """GmmLoglikesKernel<16|32|40|64|96> below the GEMM threshold: bit-exact per-Gaussian scores for dimensions on
    both sides of every instantiation's edge, frame counts round the 64-frame wave and the 256-frame block, Gaussian
    counts round the 64-Gaussian tile, padded and offset operands."""
    rng = np.random.default_rng(1000 * D + T + M)
    am = gc.clustered_model([M], D, rng)
    g, mi, iv = gc.model_params(am, oracle)
    x_host = gc.frames(rng, T, D)
    assert not gc.gemm_path(T, M, os.environ) and gc.loglikes_dp(D) == dp
    assert gc.m_per_block(T, M, dd.num_cus()) == (64, -(-M // 64))       # one trip of the mb loop per block
    x = dd.mat(x_host, 1 + (D + T) % 3, (T + M) % 2)
    gmm, views = device_model(api, g, mi, iv, am["pdf_offsets"], param_offset=M % 2)
    ll = gaussian_scores(gmm, x, pad=1 + M % 3, offset=D % 2)
    assert np.isfinite(ll).all()
    cases.exact(ll, oracle.diag_gmm_loglikes_stored(x_host, g, mi, iv))
    for v in [x] + views:
        v.assert_padding_untouched()


def test_register_kernel_rejects_97_dimensions(api, oracle, rng):
    """Above 96 dimensions and below the GEMM threshold: KH_EINVAL naming the dimension (kh_gmm.hip:513)."""
    am = gc.clustered_model([5], 97, rng)
    g, mi, iv = gc.model_params(am, oracle)
    assert gc.loglikes_dp(97) is None and not gc.gemm_path(9, 5, os.environ)
    gmm, _ = device_model(api, g, mi, iv, am["pdf_offsets"])
    x = dd.mat(gc.frames(rng, 9, 97), 1)
    out = dd.NanView(9, 5, 7, 1)
    with pytest.raises(KhError, match=r"dimension 97\b"):
        gmm.log_likelihoods(x.t, out=out.t)
    assert bool(out.buf.isnan().all())


# ---------------------------------------------------------------- b. second trip of the mb loop
def test_register_kernel_second_trip_over_the_gaussians(api, oracle, monkeypatch):
    """Enough frame blocks to fill the chip, so that LaunchLoglikes gives a block 192 of the 257 Gaussians: the mb loop
    of the register kernel runs three tiles in the first block, and two, the last of one Gaussian, in the second.
    Bit-identical to the GEMM path on the same operands, bit-exact against the oracle on the row subset."""
    import torch
    cus = dd.num_cus()
    D, M = 24, 257
    T = 256 * (2 * cus) + 5                 # frame_blocks * 2 >= 4 * cus: the Gaussians split over two blocks only
    rng = np.random.default_rng(31)
    am = gc.clustered_model([M], D, rng)
    g, mi, iv = gc.model_params(am, oracle)
    x_host = gc.frames(rng, T, D)
    x = dd.mat(x_host, 3)
    gmm, _ = device_model(api, g, mi, iv, am["pdf_offsets"])
    assert gc.gemm_path(T, M, os.environ)
    by_gemm = dd.NanView(T, M, M + 2, 1)
    gmm.log_likelihoods(x.t, out=by_gemm.t)
    monkeypatch.setenv("KH_GMM_NO_GEMM", "1")
    assert not gc.gemm_path(T, M, os.environ) and gc.loglikes_dp(D) == 32
    mpb, my = gc.m_per_block(T, M, cus)
    assert mpb >= 128 and (mpb, my) == (192, 2)
    by_regs = dd.NanView(T, M, M + 1, 0)
    gmm.log_likelihoods(x.t, out=by_regs.t)
    monkeypatch.delenv("KH_GMM_NO_GEMM")
    torch.cuda.synchronize()
    assert bool((by_regs.t.view(torch.int32) == by_gemm.t.view(torch.int32)).all())
    assert bool(by_regs.t.isfinite().all())
    rows = gc.row_subset(T)
    got = by_regs.t[torch.from_numpy(rows).cuda()].cpu().numpy()
    cases.exact(got, oracle.diag_gmm_loglikes_stored(x_host[rows], g, mi, iv))
    for v in (x, by_gemm, by_regs):
        v.assert_padding_untouched()


# ---------------------------------------------------------------- c. GEMM path
@pytest.mark.parametrize("D", [39, 40, 41, 97])
def test_gemm_path_dimensions(api, oracle, D):
    """The two-GEMM formulation just past 1 << 22 with a ragged last 64-frame block; 97 dimensions are legal here
    (only the register kernel is limited to 96)."""
    M, T = 4099, 1027
    rng = np.random.default_rng(40 + D)
    am = gc.clustered_model([M], D, rng)
    g, mi, iv = gc.model_params(am, oracle)
    x_host = gc.frames(rng, T, D)
    assert gc.gemm_path(T, M, os.environ) and not gc.gemm_path(T - 4, M, os.environ) and T % 64 != 0
    x = dd.mat(x_host, 1 + D % 3, D % 2)
    gmm, views = device_model(api, g, mi, iv, am["pdf_offsets"], param_offset=D % 2)
    ll = gaussian_scores(gmm, x)
    assert np.isfinite(ll).all()
    rows = gc.row_subset(T)
    cases.exact(ll[rows], oracle.diag_gmm_loglikes_stored(x_host[rows], g, mi, iv))
    for v in [x] + views:
        v.assert_padding_untouched()


# ---------------------------------------------------------------- d. fused kernel
def expect_tiles(off, sizes):
    tl = gc.tiles(off)
    shapes = {tuple(sizes[pb:pe]) for _, _, pb, pe in tl}
    assert {(128,), (1, 127), (127, 1), (64, 64), (100,)} <= shapes
    return tl


@pytest.mark.parametrize("tmod", [1, 40])
@pytest.mark.parametrize("D", [13, 16, 17, 39, 40])
def test_fused_kernel_on_the_edge_pdf_sizes(api, oracle, monkeypatch, D, tmod):
    """GmmFusedPdfKernel<8> (D <= 16) and <20> on tiles of one 128-Gaussian pdf, of 1 + 127, 127 + 1 and 64 + 64,
    pdfs of 1 .. 128 Gaussians that end on, before and after the chunk length, D = 16 and 40 without a zero-padded
    LDS row, D = 13, 17, 39 with the scalar tail of the 16-byte loads, ragged frame counts."""
    off, g, mi, iv, dim, rng = gc.build("edge_d%d" % D, oracle)
    M = len(g)
    T = frames_past_threshold(M, tmod)
    tl = expect_tiles(off, gc.EDGE_SIZES)
    assert gc.fused_ks(D) == (8 if D <= 16 else 20)
    split = gc.fused_split(T, len(tl), dd.num_cus(), os.environ)
    assert min(gc.share_tiles(len(tl), split)) >= 3     # both halves of the double-buffered boundaries in every share
    check_pdf_scores(api, oracle, monkeypatch, (off, g, mi, iv), gc.frames(rng, T, D), "fused_d%d_t%d" % (D, T), True,
                     rows=gc.row_subset(T), data_pad=1 + D % 3, data_offset=int(tmod == 1), param_offset=int(tmod == 40))


def test_fused_kernel_one_frame_block_a_thousand_tiles(api, oracle, monkeypatch):
    """33 frames - fewer than the 64 of a workgroup - of a model wide enough to reach 1 << 22: a single frame block
    walks more than a thousand tiles."""
    off, g, mi, iv, D, rng = gc.build("edge_wide_d13", oracle)
    T, M = 33, len(g)
    assert M >= 131072 and len(gc.tiles(off)) > 1000 and -(-T // 64) == 1
    check_pdf_scores(api, oracle, monkeypatch, (off, g, mi, iv), gc.frames(rng, T, D), "fused_wide", True,
                     rows=gc.row_subset(T), data_pad=3, param_offset=1)


@pytest.mark.parametrize("name,tiles_of_share", [("edge_d13", {"3": [12, 12, 13]}), ("edge_small_d13", {"3": [2, 2, 3]})])
def test_fused_kernel_split_of_the_tile_list(api, oracle, monkeypatch, name, tiles_of_share):
    """KH_GMM_SPLIT = 1, 3, 8 and more than there are tiles: however the tile list is shared out over blockIdx.y, the
    scores are bit-identical to the default's.  The small model has 7 tiles: the split is cut down to them."""
    off, g, mi, iv, D, rng = gc.build(name, oracle)
    M, n_tiles, cus = len(g), len(gc.tiles(off)), dd.num_cus()
    T = frames_past_threshold(M, 1)
    assert gc.fused_taken(T, D, M, off, os.environ)
    x = dd.mat(gc.frames(rng, T, D), 2)
    gmm, _ = device_model(api, g, mi, iv, off)
    base = pdf_scores(gmm, x, 4.0)
    assert np.isfinite(base).all()
    for value, want in (("1", 1), ("3", 3), ("8", min(8, n_tiles)), ("1000", min(8, n_tiles))):
        monkeypatch.setenv("KH_GMM_SPLIT", value)
        split = gc.fused_split(T, n_tiles, cus, os.environ)
        assert split == want and (value != "1000" or int(value) > n_tiles)
        if value in tiles_of_share:
            assert gc.share_tiles(n_tiles, split) == tiles_of_share[value]
        assert same_bits(pdf_scores(gmm, x, 4.0), base), value
        monkeypatch.delenv("KH_GMM_SPLIT")
    x.assert_padding_untouched()


def test_pdf_of_129_gaussians_takes_the_unfused_fallback(api, oracle, monkeypatch):
    """One pdf of 129 Gaussians among the edge sizes: BuildGmmTiles returns false and the call that would have been
    fused runs the two GEMMs and the LogSumExp row kernel."""
    off, g, mi, iv, D, rng = gc.build("edge_129_d13", oracle)
    M = len(g)
    T = frames_past_threshold(M, 40)
    assert gc.tiles(off) is None and D <= 40 and T * M >= gc.GEMM_THRESHOLD
    assert gc.gemm_path(T, M, os.environ) and gc.lse_kernel(M) == "row"
    check_pdf_scores(api, oracle, monkeypatch, (off, g, mi, iv), gc.frames(rng, T, D), "fallback_129", False,
                     rows=gc.row_subset(T), data_pad=2, data_offset=1)


# ---------------------------------------------------------------- e. LogSumExp kernel choice
@pytest.mark.parametrize("num_mix,kernel", [(1023, "thread"), (1024, "row"), (12288, "row"), (12289, "thread")])
def test_logsumexp_kernel_boundaries(api, oracle, monkeypatch, num_mix, kernel):
    """GmmPdfLseKernel against GmmPdfLseRowKernel on both sides of both boundaries of the choice, uneven pdfs of
    1 .. 200 Gaussians (two of them too large for a tile of the fused kernel)."""
    off, g, mi, iv, D, rng = gc.build("lse_%d" % num_mix, oracle)
    T = 67
    if D <= 40:
        monkeypatch.setenv("KH_GMM_NO_FUSION", "1")
    sizes = np.diff(off)
    assert len(g) == num_mix and gc.lse_kernel(num_mix) == kernel and sizes.max() == 200 and (sizes > 128).sum() == 2
    assert not gc.gemm_path(T, num_mix, os.environ) and gc.loglikes_dp(D) == (64 if D == 41 else 16)
    check_pdf_scores(api, oracle, monkeypatch, (off, g, mi, iv), gc.frames(rng, T, D), "lse_%d" % num_mix, False,
                     prunes=(-1.0, 4.0), data_pad=2, data_offset=num_mix % 2)


# ---------------------------------------------------------------- f. two slabs
def test_second_slab_of_the_unfused_path(api, oracle):
    """2^18 Gaussians: the T x M scratch is capped at 1 GiB = 1024 frames, and 1061 frames take a second slab of 37
    whose data, scratch and output pointers are offset by the first.  Rows round the slab boundary, the first and
    the last against the oracle and the float64 reference."""
    off, g, mi, iv, D, rng = gc.build("slab_d8", oracle)
    M = len(g)
    slab = gc.slab_rows(M)
    T = slab + 37
    assert M == 1 << 18 and slab == 1024 and -(-T // slab) == 2
    assert not gc.fused_taken(T, D, M, off, os.environ) and gc.tiles(off) is None
    assert gc.gemm_path(slab, M, os.environ) and gc.gemm_path(T - slab, M, os.environ) and gc.lse_kernel(M) == "thread"
    x_host = gc.frames(rng, T, D)
    rows = gc.row_subset(T, extra=(64, slab), every=None)
    assert len(rows) <= 20 and {slab - 1, slab, T - 1} <= set(rows.tolist())
    x = dd.mat(x_host, 3, 1)
    gmm, _ = device_model(api, g, mi, iv, off)
    try:
        got = pdf_scores(gmm, x, -1.0)
        assert np.isfinite(got).all()
        # the reference's input: the Gaussian scores of the 10 rows alone, a call below 1 << 22 that runs the register
        # kernel while the scores under test came from the two GEMMs; sound because ll is checked exactly against the
        # oracle here, as both paths are elsewhere (test_gemm_path_dimensions, ..._second_trip_over_the_gaussians)
        ll = gaussian_scores(gmm, dd.mat(x_host[rows], 1))
        cases.exact(ll, oracle.diag_gmm_loglikes_stored(x_host[rows], g, mi, iv))
        ref, _ = gc.lse_reference(ll, off, -1.0)
        ratio = gc.bound_ratio(got[rows], ref, off)
        assert ratio <= 1.0, ratio
        assert np.abs(got[rows] - oracle.am_gmm_loglikes(x_host[rows], g, mi, iv, off, -1.0)).max() < 1e-4
        x.assert_padding_untouched()
        print("gmm-ratio gpu slab %.3f" % ratio)
    finally:
        api.pool_release()


# ---------------------------------------------------------------- g. dictated scores
def minus_inf_pdfs(api, oracle, rng, D):
    """Three pdfs with zero weights: ComputeGconsts gives -inf there and counts them, as the oracle does."""
    w = np.array([0.5, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0, 0.0], np.float32)
    mi = rng.standard_normal((8, D)).astype(np.float32)
    iv = np.exp(0.3 * rng.standard_normal((8, D))).astype(np.float32)
    g, bad = api.gmm_compute_gconsts(w, mi, iv)
    g_o, bad_o = oracle.gmm_compute_gconsts(w, mi, iv)
    assert bad == bad_o == 5 and same_bits(g, g_o)
    assert np.array_equal(np.isneginf(g), w == 0) and np.isfinite(g[w > 0]).all()
    return {"minus_inf_inside": g[:3], "all_minus_inf": g[3:5], "minus_inf_round_one": g[5:]}


@pytest.mark.parametrize("filler", [False, True])
@pytest.mark.parametrize("D", [13, 40])
def test_dictated_scores_at_the_exact_edges(api, oracle, monkeypatch, D, filler):
    """An all-zero frame scores every Gaussian at its gconst, so each pdf's scores are dictated bit for bit: Gaussians
    exactly at and one float below the cutoff (the default one and prune = 4's), ties at the maximum, 128 equal
    scores, -inf scores inside a pdf and a pdf of nothing else (NaN, as the oracle), scores round -1e4.  Through the
    fused kernel and through the unfused path with the thread kernel (434 Gaussians) and, with 678 more of filler
    pdfs, the row kernel."""
    rng = np.random.default_rng(50 + D + filler)
    lists = gc.dictated_score_lists(rng)
    lists.update(minus_inf_pdfs(api, oracle, rng, D))
    names = list(lists)
    if filler:
        for i, n in enumerate(gc.EDGE_UNIT):
            lists["filler%d" % i] = (-50.0 + 3.0 * rng.standard_normal(n)).astype(np.float32)
    g, mi, iv, off = gc.dictated_model(list(lists.values()), D, rng)
    M, col = len(g), {k: i for i, k in enumerate(lists)}
    assert gc.lse_kernel(M) == ("row" if filler else "thread") and M == (1112 if filler else 434)
    T = frames_past_threshold(M, 1)
    gmm, _ = device_model(api, g, mi, iv, off, param_offset=1)
    zeros_fused, zeros_small = dd.mat(np.zeros((T, D), np.float32), 1), dd.mat(np.zeros((3, D), np.float32), 2, 1)
    assert gc.fused_taken(T, D, M, off, os.environ) and not gc.fused_taken(3, D, M, off, os.environ)
    ll = gaussian_scores(gmm, zeros_small)
    assert same_bits(ll, np.broadcast_to(g, ll.shape))          # the zero-frame identity on the device
    results = {}
    for prune in (-1.0, 0.0, 20.0, 4.0):
        fused = pdf_scores(gmm, zeros_fused, prune)
        plain = pdf_scores(gmm, zeros_small, prune)
        assert same_bits(fused, np.broadcast_to(fused[0], fused.shape))
        assert same_bits(plain, np.broadcast_to(fused[0], plain.shape))
        got = fused[:1]
        results[prune] = got
        ref, kept = gc.lse_reference(g[None, :], off, prune)
        assert gc.bound_ratio(got, ref, off) <= 1.0
        want = oracle.am_gmm_loglikes(np.zeros((1, D), np.float32), g, mi, iv, off, prune)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and nan.sum() == 1 and nan[0, col["all_minus_inf"]]
        big = np.zeros_like(nan)
        big[0, col["near_minus_1e4"]] = True
        assert np.abs(got - want)[~nan & ~big].max() < 1e-4
        assert abs(got[big][0] - want[big][0]) <= np.spacing(np.float32(1e4))   # floats round 1e4 are 9.8e-4 apart
        assert np.isfinite(got[~nan]).all()
        n_kept = dict(zip(lists, np.add.reduceat(kept[0].astype(np.int64), off[:-1])))
        if prune == 4.0:
            assert (n_kept["at_prune4_cutoff_kept"], n_kept["below_prune4_cutoff_dropped"]) == (2, 1)
            assert n_kept["at_prune4_cutoff_chunk2"] == 10
        else:
            assert (n_kept["at_cutoff_kept"], n_kept["below_cutoff_dropped"]) == (121, 1)
    assert same_bits(results[0.0], results[-1.0]) and same_bits(results[20.0], results[-1.0])
    r = results[-1.0][0]
    assert r[col["below_cutoff_dropped"]] == np.float32(0.25) and r[col["single"]] == np.float32(-17.0)
    assert r[col["at_cutoff_kept"]] > np.float32(0.25)
    assert results[4.0][0][col["below_prune4_cutoff_dropped"]] == np.float32(0.25)
    assert abs(float(r[col["equal_128"]]) - (-42.5 + np.log(128.0))) <= gc.lse_bound(np.array([[-37.6]]), [0, 128])[0, 0]
    assert names[0] == "at_cutoff_kept"
    for v in (zeros_fused, zeros_small):
        v.assert_padding_untouched()


# ---------------------------------------------------------------- h. contract of pdf_offsets
def bad_offsets(off):
    """name -> (offsets that do not run strictly increasing from 0 to num_mix yet stay inside the arrays, the pdf the
    message must name)."""
    P = len(off) - 1
    empty = off.copy()
    empty[50] = empty[49]                      # pdf 49 empty (pdf 49 of 128 one-Gaussian pdfs: the tile's 129th entry)
    back = off.copy()
    back[130] = back[129] - 1
    first = off.copy()
    first[0] = 1
    last = off.copy()
    last[-1] -= 1
    return {"empty": (empty, 49), "backwards": (back, 129), "first": (first, 0), "last": (last, P - 1)}


@pytest.mark.parametrize("which", ["empty", "backwards", "first", "last"])
@pytest.mark.parametrize("path", ["fused", "unfused"])
def test_pdf_offsets_contract(api, oracle, path, which):
    """Offsets with an empty pdf, a pdf running backwards, a first entry other than 0 or a last one other than
    num_mix are rejected on both paths with a message naming the pdf, before any kernel indexes with them; nothing
    is written.  Every offset stays inside the parameter arrays."""
    rng = np.random.default_rng(60)
    sizes = [1] * 128 + gc.EDGE_UNIT
    am = gc.clustered_model(sizes, 13, rng)
    g, mi, iv = gc.model_params(am, oracle)
    off = am["pdf_offsets"]
    M = len(g)
    T = frames_past_threshold(M, 1) if path == "fused" else 5
    assert gc.fused_taken(T, 13, M, off, os.environ) == (path == "fused")
    bad, pdf = bad_offsets(off)[which]
    assert bad.min() >= 0 and bad.max() <= M and len(bad) == len(off) and not np.array_equal(bad, off)
    x = dd.mat(gc.frames(rng, T, 13), 1)
    gmm, _ = device_model(api, g, mi, iv, bad)
    out = dd.NanView(T, gmm.num_pdfs, gmm.num_pdfs + 2, 1)
    with pytest.raises(KhError, match=r"pdf %d\b" % pdf):
        gmm.pdf_log_likelihoods(x.t, out=out.t)
    assert bool(out.buf.isnan().all())
    good, _ = device_model(api, g, mi, iv, off)
    assert np.isfinite(pdf_scores(good, x, -1.0)).all()     # the same call with the model's own offsets goes through


def test_no_frames_is_the_references_assertion(api, oracle, rng):
    """T = 0: KALDI_ASSERT(data.NumRows() != 0) of DiagGmm::LogLikelihoods on both entry points, from the library
    itself as well (a view of no rows over a non-empty buffer)."""
    import torch
    am = gc.clustered_model([3, 4], 13, rng)
    g, mi, iv = gc.model_params(am, oracle)
    gmm, _ = device_model(api, g, mi, iv, am["pdf_offsets"])
    empty = torch.empty((0, 13), dtype=torch.float32, device="cuda")
    for call in (gmm.pdf_log_likelihoods, gmm.log_likelihoods):
        with pytest.raises(KhError, match=r"data\.NumRows\(\) != 0"):
            call(empty)
    lib, capi = api.lib(), importlib.import_module("old-kaldi-git_amd.capi")
    buf, out = torch.zeros((4, 13), device="cuda"), torch.zeros((4, 2), device="cuda")
    rc = lib.kh_am_gmm_loglikes(api._p(buf), capi.KhMatrixDim(0, 13, 13), api._p(gmm.gconsts), api._p(gmm.means_invvars),
                                api._p(gmm.inv_vars), api._p(gmm.pdf_offsets), 2, 7, -1.0, api._p(out), 2)
    assert rc != 0 and "data.NumRows() != 0" in lib.kh_last_error().decode()
