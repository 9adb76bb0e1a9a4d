"""CPU: the fMLLR restatement (tests/fmllr_restatement.py) against the oracle where the oracle speaks, the library's host-side
update (kh_fmllr_update needs no device) against the restatement, the host posterior / transform algebra of api.py, and the
measured end-to-end tolerance of tests/fmllr_cases.py."""
import numpy as np
import pytest

import fmllr_cases as C
import fmllr_restatement as R
from conftest import pkg


@pytest.fixture(scope="module")
def e2e(oracle):
    return C.e2e_reference(oracle)


def test_scores_equal_the_oracle_bit_for_bit(oracle):
    """A1's per-Gaussian scores: the restatement's fmaf chains are the oracle's (and kh_gmm.hip's)."""
    for am, feats in ((C.a1_case(oracle)[0], C.a1_case(oracle)[1]), C.e2e_case(oracle)[:2]):
        feats = feats[:40]
        want = oracle.diag_gmm_loglikes_stored(feats, am["gconsts"], am["means_invvars"], am["inv_vars"])
        got = np.stack([R.scores(x, am["gconsts"], am["means_invvars"], am["inv_vars"]) for x in feats])
        assert np.array_equal(want.view(np.int32), got.view(np.int32))


def test_fmaf_rounds_once():
    """The emulated fmaf against exact rational arithmetic, on operands made to tie at the float64 sum."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(2000).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (rng.standard_normal(2000) * np.exp(rng.uniform(-30, 30, 2000))).astype(np.float32)
    a[:3], b[:3] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23)
    c[:3] = np.float32([2.0 ** -70, -2.0 ** -70, 0.0])      # 1 + 2^-22 + 2^-46 +- tiny: the float64 sum ties without the fix
    got = R.fmaf(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i


def test_soft_max_sums_to_the_weight(oracle):
    am, feats, posts = C.a1_case(oracle)
    ent = R.entries_of(posts, am["pdf_offsets"])
    post, like = R.component_posteriors(am, feats, ent)
    for e in range(len(ent["pdf"])):
        p = post[ent["goff"][e]:ent["goff"][e + 1]].astype(np.float64)
        assert abs(p.sum() - ent["weight"][e]) <= 1e-5 * max(1, len(p)) and np.isfinite(like[e])


def test_merged_frames_of_the_a2_case(oracle):
    """The merging rule on the case that holds every instance of it (tests/fmllr_cases.py a2_case)."""
    am, feats, utt, spk, gposts = C.a2_case(oracle)
    ent, _ = C.gpost_entries(gposts)
    run_row, run_entry, spk_run = R.merged_frames(feats, utt, spk, ent["feo"])
    assert run_row.tolist() == [0, 1, 4, 7, 8, 10, 11, 12, 13, 14, 15, 16, 20, 21, 22, 23]
    assert spk_run.tolist() == [0, 6, 13, 16]


def test_library_update_matches_the_restatement(e2e):
    """kh_fmllr_update (host C++) on the restatement's statistics: every update type, the speaker under the min-count."""
    api = pkg("api")
    st = e2e["stats"]
    for ty in C.TYPES:
        w_ref, impr_ref, count_ref = e2e["ref"][ty]
        W, impr, count = api.fmllr_update(st, ty, C.E2E_MIN_COUNT, 40)
        tol = C.transform_tolerance(w_ref, ty)
        err = np.abs(W.astype(np.float64) - w_ref)
        print(ty, "max err", err.max(), "tolerance", tol.min(), "impr", impr, impr_ref)
        assert (err <= tol).all(), ty
        assert np.array_equal(count, count_ref)
        assert np.allclose(impr, impr_ref, rtol=1e-4, atol=1e-3)      # float differences of two ~1e3 objective values
        assert np.array_equal(W[3], np.eye(13, 14, dtype=np.float32)) and impr[3] == 0.0 and count[3] < C.E2E_MIN_COUNT
        for s in range(3):
            Gf = R.full_g(st["G"][s], 13)
            f_ref = R.aux(w_ref[s], st["beta"][s], st["K"][s], Gf)
            f_got = R.aux(W[s], st["beta"][s], st["K"][s], Gf)
            assert f_got >= f_ref - C.aux_drop_allowed(w_ref[s], tol[s], st["beta"][s], st["K"][s], st["G"][s]), (ty, s)
    with pytest.raises(api.KhError, match="Unknown fMLLR update type"):
        api.fmllr_update(st, "fulll")


def test_update_single_thread_equals_threads(e2e):
    api = pkg("api")
    a = api.fmllr_update(e2e["stats"], "full", C.E2E_MIN_COUNT, 40, num_threads=1)
    b = api.fmllr_update(e2e["stats"], "full", C.E2E_MIN_COUNT, 40, num_threads=16)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_measured_tolerance_is_what_is_recorded(e2e, oracle):
    """fmllr_cases.MEASURED_DIFF is the figure this machine measures, within a factor 2 (the linear algebra under numpy)."""
    print("measured", e2e["diff"], "recorded", C.MEASURED_DIFF, "seed", C.TOL_SEED)
    for ty in C.TYPES:
        m, r = e2e["diff"][ty], C.MEASURED_DIFF[ty]
        assert m <= 2 * r and r <= 2 * max(m, 2.0 ** -24), ty
    m, r = C.e2e_reference(oracle, per_utt=True)["diff"]["full"], C.MEASURED_DIFF_PER_UTT["full"]
    print("per utterance: measured", m, "recorded", r)
    assert m <= 2 * r and r <= 2 * m


def test_e2e_case_is_what_the_issue_asks(e2e):
    st = e2e["stats"]
    assert (st["beta"][:3] >= 30 * 14).all() and st["beta"][3] < C.E2E_MIN_COUNT
    fs = e2e["fs"]
    assert fs["spk_run_offsets"][-1] < np.count_nonzero(np.diff(e2e["ent"]["feo"]))      # some rows did merge


def test_weight_silence_post():
    api = pkg("api")
    tid2phone = np.array([0, 1, 1, 2, 2, 3, 3], np.int32)
    post = [[(1, 1.0)], [(3, 0.25), (1, 0.75)], [], [(5, 0.5), (4, 0.5)], [(2, 0.0)], [(1, 0.3), (2, 0.7)]]
    for scale in (0.0, 0.01, 1.0):
        for dist in (False, True):
            got = api.weight_silence_post(tid2phone, [1], scale, post, distribute=dist)
            assert got == R.weight_silence_post(tid2phone, [1], scale, post, distribute=dist)
    got = api.weight_silence_post(tid2phone, [1], 0.0, post)
    assert got[0] == [] and got[1] == [(3, 0.25)] and got[3] == post[3] and got[5] == []
    got = api.weight_silence_post(tid2phone, [1], 0.0, post, distribute=True)
    assert got[0] == [] and got[1] == [(3, 0.0625), (1, 0.1875)] and got[4] == post[4]     # a zero frame is left as it is


def test_compose_transforms(rng):
    api = pkg("api")
    a = rng.standard_normal((13, 14)).astype(np.float32)
    for b, aff in ((rng.standard_normal((14, 9)), False), (rng.standard_normal((13, 40)), False), (rng.standard_normal((13, 41)), True)):
        b = b.astype(np.float32)
        got = api.compose_transforms(a, b, aff)
        want = R.compose_transforms(a, b, aff)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-4
    assert api.compose_transforms(a, np.zeros((0, 3), np.float32)) is None
    with pytest.raises(api.KhError, match="mismatched dimensions"):
        api.compose_transforms(a, rng.standard_normal((11, 4)).astype(np.float32))
