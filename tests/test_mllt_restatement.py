"""No GPU: tests/mllt_restatement.py itself, the exact sums of tests/mllt_cases.py, and the library's host RandPrune
(kh_rand_prune, which needs no device) against the restatement's, bit for bit and draw for draw."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import mllt_cases as C
import mllt_restatement as M
from conftest import pkg

F32 = np.float32


def test_rand_prune_cases_of_the_reference():
    """base/kaldi-math-test.cc:144-155."""
    assert M.rand_prune(1.1, 1.0) == F32(1.1)
    assert M.rand_prune(0.0, 0.0) == 0.0
    assert M.rand_prune(-1.1, 1.0) == F32(-1.1)
    assert M.rand_prune(0.0, 1.0) == 0.0
    assert M.rand_prune(0.5, 1.0) >= 0.0
    assert M.rand_prune(-0.5, 1.0) <= 0.0
    for _ in range(20):
        assert M.rand_prune(-0.5, 1.0) in (0.0, -1.0)
        assert M.rand_prune(0.5, 1.0) in (0.0, 1.0)
    with pytest.raises(AssertionError):
        M.rand_prune(0.5, -1.0)


def test_draws_are_the_c_librarys():
    """After srand(1) - the state of a process that never seeds - rand() gives the C library's default sequence, and
    RandUniform is the float of (rand() + 1.0) / (RAND_MAX + 2.0)."""
    M.srand(1)
    assert [M.rand(), M.rand()] == [1804289383, 846930886]
    M.srand(1)
    assert M.rand_uniform() == F32((1804289383 + 1.0) / (2147483647 + 2.0))
    assert ctypes.CDLL(None).rand() == 846930886                     # the module draws from the process's one generator


def test_no_draw_at_threshold_zero():
    M.srand(7)
    want = [M.rand() for _ in range(3)]
    M.srand(7)
    before = M.DRAWS[0]
    vals = [F32(v) for v in (0.3, -0.2, 0.0, -0.0, 1e-30, 5.0)]
    assert [M.rand_prune(v, 0.0) for v in vals] == vals
    assert M.DRAWS[0] == before
    assert [M.rand() for _ in range(3)] == want                      # the state after equals the state before


def test_exact_sums_and_the_restatements_own_bound():
    """math.fsum on the split addends is the rational sum rounded once; the restatement's frame-order sums are within the
    bound of it (every element, D = 5 and D = 3)."""
    for dim, n, seed in ((5, 40, 3), (3, C.CHUNK + 1, 4)):
        c = C.kernel_case(dim, n, seed)
        o, w, p = C.items_of(c["off"], c["mi"], c["iv"], c["feats"], c["ent"], c["post"])
        assert len(o) == n
        picks = C.picks_of(dim, 0)
        assert len(picks) == dim * dim * (dim + 1) // 2
        fs, ra = C.exact_elements(o, w, picks), C.exact_elements_rational(o, w, picks)
        for (s, m), (rs, rm) in zip(fs, ra):
            assert s == float(rs) and m == float(rm)                 # float(Fraction) rounds to nearest even, once
        acc = M.init_accs(dim, 0.0)
        am = dict(pdf_offsets=c["off"], means_invvars=c["mi"], inv_vars=c["iv"])
        before = M.DRAWS[0]
        M.accumulate_entries(acc, am, c["feats"], c["ent"], c["post"])
        assert M.DRAWS[0] == before                                  # rand_prune = 0: no draw
        print("D", dim, "n", n, "restatement worst error / bound", C.check_bound(acc["G"], o, w, dim, 0, "restatement"))
        want_beta = 0.0
        for e in range(len(c["ent"]["pdf"])):
            s = 0.0
            for v in c["post"][int(c["ent"]["goff"][e]):int(c["ent"]["goff"][e + 1])]:
                if v != 0:
                    s += float(v)
            want_beta += s
        assert acc["beta"] == want_beta
        assert abs(Fraction(acc["beta"]) - sum(Fraction(float(v)) for v in p)) <= (n + 2) * Fraction(2) ** -53 * sum(abs(Fraction(float(v))) for v in p)


def test_slice_plan():
    assert C.slice_plan(0, 40) == (0, 0, 0)
    assert C.slice_plan(1, 2) == (C.CHUNK, 1, 1)
    assert C.slice_plan(2 * C.CHUNK + 1, 40) == (C.CHUNK, 3, 3 * 4)                    # Q = 820: 52 tiles, 4 groups of 16
    assert C.slice_plan(C.CHUNK * C.MAX_SLICES, 31) == (C.CHUNK, C.MAX_SLICES, C.MAX_SLICES * 2)   # Q = 496: 31 tiles
    assert C.slice_plan(C.CHUNK * C.MAX_SLICES + 1, 2) == (2 * C.CHUNK, C.MAX_SLICES // 2 + 1, C.MAX_SLICES // 2 + 1)


def test_margins_condition():
    assert C.margins_hold([(0.5, 0.25, None, None), (0.1, 0.25, 0.7, 0.4), (0.25, 0.25, None, None)])
    assert not C.margins_hold([(0.1, 0.25, float(np.nextafter(F32(0.4), F32(1))), float(F32(0.4)))])
    assert not C.margins_hold([(float(np.nextafter(F32(0.25), F32(1))), 0.25, None, None)])


# ---------------------------------------------------------------- kh_rand_prune: host code of the library, no device
@pytest.fixture(scope="module")
def lib():
    return pkg("capi").load()


def kh_rand_prune(lib, post, thresh, seed=None):
    capi = pkg("capi")
    return lib.kh_rand_prune(post.ctypes.data_as(capi.c_float_p), post.size, float(thresh), 0 if seed is None else 1, 0 if seed is None else seed)


@pytest.mark.parametrize("thresh", [0.25, 4.0, 1.0, 0.0])
def test_kh_rand_prune_equals_the_restatement(lib, thresh):
    rng = np.random.default_rng(17)
    t = F32(thresh)
    vals = np.concatenate([rng.uniform(-1.2, 1.2, 3000) * rng.choice([1.0, 0.1, 1e-3, 1e-6], 3000), [0.0, -0.0, thresh, -thresh],
                           [np.nextafter(t, F32(0)), -np.nextafter(t, F32(0)), np.nextafter(t, F32(9)), 1e-42, -1e-42]]).astype(F32)
    rng.shuffle(vals)
    M.srand(123)
    before = M.DRAWS[0]
    want = np.array([M.rand_prune(v, thresh) for v in vals], F32)
    draws = M.DRAWS[0] - before
    tail = M.rand()
    got = vals.copy()
    assert kh_rand_prune(lib, got, thresh, seed=123) == 0
    assert np.array_equal(got.view(np.int32), want.view(np.int32))                   # equal bits: -0.0 for a negative value pruned away
    M.srand(123)
    again = vals.copy()
    assert kh_rand_prune(lib, again, thresh, seed=None) == 0                        # no reseed: draws on from the process's state
    assert np.array_equal(again.view(np.int32), want.view(np.int32))
    assert ctypes.CDLL(None).rand() == tail                                          # the same number of draws
    expect = int(((vals != 0) & (np.abs(vals) < t)).sum())
    assert draws == expect and (thresh != 0.0 or draws == 0)
    if thresh == 4.0:
        assert set(np.abs(got[got != 0]).tolist()) == {4.0, float(np.nextafter(t, F32(9)))}     # the one input above the threshold
    if thresh == 0.0:
        assert np.array_equal(got.view(np.int32), vals.view(np.int32))


def test_kh_rand_prune_refuses_a_negative_threshold(lib):
    capi = pkg("capi")
    v = np.array([0.5], F32)
    assert kh_rand_prune(lib, v, -1.0) == -1                          # KH_EINVAL
    assert b"prune threshold -1" in lib.kh_last_error() and v[0] == F32(0.5)
    assert kh_rand_prune(lib, np.zeros(0, F32), 0.25) == 0


def test_api_rand_prune(lib):
    api = pkg("api")
    v = np.array([0.1, -0.1, 0.5, 0.0], F32)
    M.srand(5)
    want = np.array([M.rand_prune(x, 0.25) for x in v], F32)
    out = api.rand_prune(v, 0.25, seed=5)
    assert out is v and np.array_equal(v.view(np.int32), want.view(np.int32))
    with pytest.raises(api.KhError, match="float32"):
        api.rand_prune(np.zeros(3), 0.25)
    with pytest.raises(api.KhError, match="prune threshold"):
        api.rand_prune(v, -0.5)


def test_kh_rand_prune_at_positions_the_generator(lib):
    """srand(seed), skip, prune: one call and the same array cut into three calls, each skipping the draws of those before,
    give the restatement's bits - whatever was drawn from the generator in between."""
    capi = pkg("capi")
    rng = np.random.default_rng(23)
    vals = (rng.uniform(-1.0, 1.0, 2000) * rng.choice([1.0, 0.1, 0.0], 2000)).astype(F32)
    M.srand(1)
    before = M.DRAWS[0]
    want = np.array([M.rand_prune(v, 0.25) for v in vals], F32)
    total = M.DRAWS[0] - before

    def at(a, seed, skip):
        d = ctypes.c_int64(-1)
        assert lib.kh_rand_prune_at(a.ctypes.data_as(capi.c_float_p), a.size, 0.25, seed, skip, ctypes.byref(d)) == 0
        return int(d.value)
    M.srand(99)                                                          # someone else reseeds
    got = vals.copy()
    assert at(got, 1, 0) == total and np.array_equal(got.view(np.int32), want.view(np.int32))
    parts, skip = [vals[:700].copy(), vals[700:701].copy(), vals[701:].copy()], 0
    for part in parts:
        M.rand(), M.srand(skip + 5)                                      # and draws, between the calls
        skip += at(part, 1, skip)
    assert skip == total and np.array_equal(np.concatenate(parts).view(np.int32), want.view(np.int32))
    api = pkg("api")
    again = vals.copy()
    assert api.rand_prune_at(again, 0.25, 1, 0) == total and np.array_equal(again.view(np.int32), want.view(np.int32))
    d = ctypes.c_int64(0)
    assert lib.kh_rand_prune_at(got.ctypes.data_as(capi.c_float_p), got.size, -0.5, 1, 0, ctypes.byref(d)) == -1
    assert lib.kh_rand_prune_at(got.ctypes.data_as(capi.c_float_p), got.size, 0.5, 1, -1, ctypes.byref(d)) == -1
