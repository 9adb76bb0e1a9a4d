"""The references of test_gpu_gmm_dispatch.py checked on the CPU before anything trusts them (tests/gmm_cases.py):
the float64 LogSumExp against the oracle inside the derived bound on every model of the GPU module, the zero-frame
identity that lets a test dictate a pdf's scores, the invariants of the restated tile list, and the sensitivity
condition: on the unpruned clustered models no pdf may degenerate to its maximum - removing its first Gaussian, its
last, or the first one the fused kernel's chunk loop reads must move the reference by more than the bound."""
import numpy as np
import pytest

import gmm_cases as gc

T_CPU = 70
MODELS = sorted(gc.lse_models())


@pytest.fixture(scope="module")
def scored(oracle):
    """name -> (offsets, ll [T_CPU, M] of the oracle, the model and the frames), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            off, g, mi, iv, dim, rng = gc.build(name, oracle)
            x = gc.frames(rng, 24 if len(g) > 100000 else T_CPU, dim)
            cache[name] = (off, oracle.diag_gmm_loglikes_stored(x, g, mi, iv), (g, mi, iv), x)
        return cache[name]
    return get


@pytest.mark.parametrize("name", MODELS)
def test_float64_logsumexp_against_the_oracle(oracle, scored, name):
    """The oracle (float expf, double log) stays inside the bound derived for the kernels, for every prune the GPU
    module uses, and the project's 1e-4 holds with it."""
    off, ll, (g, mi, iv), x = scored(name)
    worst = 0.0
    for prune in (-1.0, 4.0, 0.5):
        ref, kept = gc.lse_reference(ll, off, prune)
        assert np.isfinite(ref).all()
        got = oracle.am_gmm_loglikes(x, g, mi, iv, off, prune)
        ratio = gc.bound_ratio(got, ref, off)
        worst = max(worst, ratio)
        assert np.abs(got - ref).max() < 1e-4
        if prune == 0.5:   # the pruning bites: the kept set is smaller than the default cutoff's
            assert kept.sum() < gc.lse_reference(ll, off, -1.0)[1].sum()
    print("gmm-ratio oracle %s %.3f" % (name, worst))
    assert worst <= 1.0, worst


def test_bound_constant():
    """c(n) as the docstring of gmm_cases.py states it."""
    assert abs(gc.lse_c(128) - 2.63e-6) < 1e-8 and abs(gc.lse_c(1) - 1.82e-6) < 1e-8
    assert (np.diff(gc.lse_c(np.arange(1, 20000))) >= 0).all()
    assert gc.MIN_LOG_DIFF == np.log(np.float32(2.0 ** -23)) and abs(float(gc.MIN_LOG_DIFF) + 15.9424) < 1e-4


def test_zero_frame_identity_on_the_oracle(oracle, rng):
    """An all-zero frame scores every Gaussian at its gconst, bit for bit (-inf included), so a test dictates scores."""
    lists = list(gc.dictated_score_lists(rng).values()) + [np.array([-np.inf, -3.0, -np.inf], np.float32),
                                                           np.array([-np.inf] * 3, np.float32)]
    for dim in (13, 40):
        g, mi, iv, off = gc.dictated_model(lists, dim, rng)
        ll = oracle.diag_gmm_loglikes_stored(np.zeros((3, dim), np.float32), g, mi, iv)
        assert np.array_equal(ll.view(np.int32), np.broadcast_to(g, ll.shape).view(np.int32))


def test_dictated_cases_discriminate(oracle, rng):
    """The dictated pdfs decide what they are about: kept and dropped differ by more than twice the bound in the
    reference, and the oracle agrees with the reference on each."""
    d = gc.dictated_score_lists(rng)
    names = list(d)
    g, mi, iv, off = gc.dictated_model([d[k] for k in names], 13, rng)
    ll = np.broadcast_to(g, (2, len(g)))
    res = {}
    for prune in (-1.0, 4.0):
        ref, kept = gc.lse_reference(ll, off, prune)
        got = oracle.am_gmm_loglikes(np.zeros((2, 13), np.float32), g, mi, iv, off, prune)
        assert gc.bound_ratio(got, ref, off) <= 1.0
        per_pdf_kept = np.add.reduceat(kept[0].astype(np.int64), off[:-1])
        res[prune] = {k: (ref[0, i], gc.lse_bound(ref, off)[0, i], int(per_pdf_kept[i])) for i, k in enumerate(names)}
    a, b = res[-1.0]["at_cutoff_kept"], res[-1.0]["below_cutoff_dropped"]
    assert a[2] == 121 and b[2] == 1 and b[0] == 0.25
    assert a[0] - b[0] > a[1] + b[1]   # no result is inside both bounds
    a, b = res[4.0]["at_prune4_cutoff_kept"], res[4.0]["below_prune4_cutoff_dropped"]
    assert a[2] == 2 and b[2] == 1 and a[0] - b[0] > 1e-2
    assert res[4.0]["at_prune4_cutoff_chunk2"][2] == 10 and res[-1.0]["at_prune4_cutoff_chunk2"][2] == 19
    assert res[-1.0]["tie_at_max"][2] == 4
    e = res[-1.0]["equal_128"]
    assert abs(e[0] - (-42.5 + np.log(128.0))) < 1e-12


SIZE_LISTS = {
    "edge": gc.EDGE_SIZES, "edge_small": gc.EDGE_SIZES_SMALL, "edge_129": gc.EDGE_SIZES_129, "ones": [1] * 300,
    "full": [128] * 3, "too_big": [129], "too_big_last": [5, 128, 129], "one": [1], "just": [127, 2, 126, 1, 1, 128],
    "random": [int(v) for v in np.random.default_rng(7).integers(1, 129, 500)],
    "random_big": [int(v) for v in np.random.default_rng(8).integers(1, 140, 200)],
}


@pytest.mark.parametrize("name", sorted(SIZE_LISTS))
def test_restated_tiles_invariants(name):
    sizes = SIZE_LISTS[name]
    off = gc.offsets_of(sizes)
    tl = gc.tiles(off)
    assert (tl is None) == (max(sizes) > gc.KGT)
    if tl is None:
        return
    p = 0
    for mb, me, pb, pe in tl:
        assert pb == p and pe > pb                      # whole pdfs, in order, none skipped
        assert mb == off[pb] and me == off[pe]          # the tile's Gaussians are exactly its pdfs'
        assert 0 < me - mb <= gc.KGT
        assert pe == len(sizes) or off[pe + 1] - mb > gc.KGT   # greedy: the next pdf did not fit
        p = pe
    assert p == len(sizes)


def test_edge_list_holds_the_edges_it_names():
    off = gc.offsets_of(gc.EDGE_SIZES)
    tl = gc.tiles(off)
    shapes = {tuple(int(off[p + 1] - off[p]) for p in range(pb, pe)) for _, _, pb, pe in tl}
    for want in ((128,), (1, 127), (127, 1), (64, 64), (100,)):
        assert want in shapes, want
    assert any(a == 128 and b == 1 for a, b in zip(gc.EDGE_SIZES, gc.EDGE_SIZES[1:]))
    assert set(gc.EDGE_SIZES) >= {1, 7, 8, 9, 16, 17, 100, 128}
    assert min(gc.share_tiles(len(tl), 8)) >= 3         # both parities of the boundary double buffer in every share
    assert len(gc.tiles(gc.offsets_of(gc.EDGE_SIZES_SMALL))) == 7
    assert gc.tiles(gc.offsets_of(gc.EDGE_SIZES_129)) is None and gc.EDGE_SIZES_129.count(129) == 1


def test_restated_decisions_at_their_edges():
    assert [gc.loglikes_dp(d) for d in (1, 16, 17, 32, 33, 40, 41, 64, 65, 96, 97)] == \
        [16, 16, 32, 32, 40, 40, 64, 64, 96, 96, None]
    assert [gc.lse_kernel(n) for n in (1023, 1024, 12288, 12289)] == ["thread", "row", "row", "thread"]
    assert gc.slab_rows(1 << 18) == 1024 and gc.slab_rows(9000) == (1 << 28) // 9000 and gc.slab_rows(1 << 27) == 64
    assert gc.m_per_block(257, 700, 256) == (64, 11) and gc.m_per_block(256 * 512 + 5, 257, 256) == (192, 2)
    assert gc.fused_split(1089, 37, 256, {}) == 8 and gc.fused_split(1089, 37, 256, {"KH_GMM_SPLIT": "3"}) == 3
    assert gc.fused_split(6209, 7, 256, {"KH_GMM_SPLIT": "1000"}) == 7 and gc.fused_split(70000, 37, 256, {}) == 8
    assert gc.fused_split(1 << 20, 37, 256, {}) == 1 and gc.fused_split(64, 37, 256, {"KH_GMM_SPLIT": "0"}) == 1
    assert gc.share_tiles(7, 3) == [2, 2, 3]
    off = gc.offsets_of(gc.EDGE_SIZES)
    assert gc.fused_taken(1089, 40, 4068, off, {}) and not gc.fused_taken(1089, 41, 4068, off, {})
    assert not gc.fused_taken(1031, 40, 4068, off, {}) and not gc.fused_taken(1089, 40, 4068, off, {"KH_GMM_NO_FUSION": "1"})
    assert (gc.fused_ks(16), gc.fused_ks(17)) == (8, 20)


@pytest.mark.parametrize("name", MODELS)
def test_sensitivity_every_gaussian_counts(scored, name):
    """Without pruning, removing the first, the last or (where it exists) the ninth Gaussian of any pdf of two or more
    moves the float64 reference by more than the bound on at least 25 % of the frames: a kernel that dropped one, or
    set a pdf boundary off by one, cannot hide below the tolerance."""
    off, ll, _, _ = scored(name)
    ref, kept = gc.lse_reference(ll, off, -1.0)
    bound = gc.lse_bound(ref, off)
    sizes = np.diff(off)
    ll64 = ll.astype(np.float64)
    worst = 1.0
    for which in ("first", "last", "ninth"):
        pdfs = np.nonzero(sizes >= (9 if which == "ninth" else 2))[0]
        col = {"first": off[pdfs], "last": off[pdfs + 1] - 1, "ninth": off[pdfs] + 8}[which]
        # ref = log(sum of kept exp(ll)); without Gaussian g: log(exp(ref) - exp(ll_g)) = ref + log1p(-exp(ll_g - ref))
        share = np.where(kept[:, col], np.exp(ll64[:, col] - ref[:, pdfs]), 0.0)
        moved = -np.log1p(-np.minimum(share, 1.0 - 1e-16))
        frac = (moved > bound[:, pdfs]).mean(axis=0)
        worst = min(worst, float(frac.min()))
        assert frac.min() >= 0.25, (which, int(pdfs[frac.argmin()]), int(sizes[pdfs[frac.argmin()]]), float(frac.min()))
    print("gmm-sensitivity %s %.2f" % (name, worst))
