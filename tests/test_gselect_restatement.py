"""No GPU: tests/gselect_restatement.py on hand cases with the answers written out.  Most models here have means_invvars = 0 and
inv_vars = 0, so a Gaussian's score IS its gconst in both modes and every order can be read off the numbers."""
import math

import numpy as np
import pytest

import gselect_restatement as R

F32 = np.float32
MODES = ["library", "reference"]


def flat_model(gconsts, dim=1):
    g = np.asarray(gconsts, F32)
    return dict(gconsts=g, means_invvars=np.zeros((len(g), dim), F32), inv_vars=np.zeros((len(g), dim), F32))


def random_model(seed, G, D):
    rng = np.random.default_rng(seed)
    iv = rng.uniform(0.5, 2.0, (G, D)).astype(F32)
    mi = (rng.standard_normal((G, D)) * iv).astype(F32)
    return dict(gconsts=rng.uniform(-8, -4, G).astype(F32), means_invvars=mi, inv_vars=iv)


X = np.asarray([0.75], F32)


@pytest.mark.parametrize("mode", MODES)
def test_two_identical_gaussians_larger_index_first(mode):
    out, like, st = R.gaussian_selection_frame(flat_model([1, 3, 3, 0]), X, 2, mode)
    assert out == [2, 1] and st == 0
    assert like == F32(F32(3) + F32(math.log1p(1.0)))          # LogAdd(3, 3) = 3 + Log1p(Exp(0))
    assert like == F32(3.6931472)


@pytest.mark.parametrize("mode", MODES)
def test_all_scores_equal(mode):
    assert R.gaussian_selection_frame(flat_model([2, 2, 2, 2]), X, 2, mode)[0] == [3, 2]
    assert R.gaussian_selection_frame(flat_model([2, 2, 2, 2]), X, 4, mode)[0] == [3, 2, 1, 0]


@pytest.mark.parametrize("mode", MODES)
def test_more_than_n_scores_reach_the_threshold(mode):
    """thresh = 5 and three scores are >= it: the sort decides which two stay."""
    assert R.gaussian_selection_frame(flat_model([5, 1, 5, 5]), X, 2, mode)[0] == [3, 2]


@pytest.mark.parametrize("mode", MODES)
def test_positive_and_negative_zero_tie(mode):
    assert R.gaussian_selection_frame(flat_model([-0.0, 0.0, -1]), X, 2, mode)[0] == [1, 0]
    assert R.gaussian_selection_frame(flat_model([0.0, -0.0, -1]), X, 2, mode)[0] == [1, 0]
    # (a gconst of -0 plus the chain's +0 is +0, so the model cannot carry the sign to the comparison: the rule itself)
    assert R.select(np.asarray([-0.0, 0.0, -1], F32), [0, 1, 2], 2)[0] == [1, 0]
    assert R.select(np.asarray([0.0, -0.0, -1], F32), [0, 1, 2], 2)[0] == [1, 0]
    assert R.select(np.asarray([0.0, -0.0, 1e-45], F32), [0, 1, 2], 1)[0] == [2]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,want", [(1, [2]), (3, [2, 3, 0]), (4, [2, 3, 0, 1]), (7, [2, 3, 0, 1])], ids=["1", "G-1", "G", "n>G"])
def test_n_against_the_number_of_gaussians(mode, n, want):
    assert R.gaussian_selection_frame(flat_model([0.5, -1, 2, 1]), X, n, mode)[0] == want


def test_log_add_chain():
    """The first step from -inf returns the score itself; a score more than -Log(FLT_EPSILON) below the total adds nothing."""
    assert R.log_add(F32(-np.inf), F32(-7.25)) == F32(-7.25)
    assert R.log_add(F32(-np.inf), F32(-np.inf)) == F32(-np.inf)
    assert R.MIN_LOG_DIFF_FLOAT == F32(-15.942385)
    assert R.log_add(F32(5), F32(-11)) == F32(5)                                     # diff -16 < kMinLogDiffFloat
    assert R.log_add(F32(5), F32(-10.5)) == F32(F32(5) + F32(math.log1p(float(F32(math.exp(-15.5))))))
    assert R.log_add(F32(1), F32(2)) == R.log_add(F32(2), F32(1)) == F32(F32(2) + F32(math.log1p(float(F32(math.exp(-1.0))))))
    out, like, _ = R.gaussian_selection_frame(flat_model([-7.25, -30]), X, 1)
    assert out == [0] and like == F32(-7.25)
    out, like, _ = R.gaussian_selection_frame(flat_model([5, -11, -30]), X, 2)
    assert out == [0, 1] and like == F32(5)


@pytest.mark.parametrize("mode", MODES)
def test_preselection(mode):
    m = flat_model([0.5, 4, 4, 1, -2])
    # shorter than n: this_num_gselect = the list's size; the order is by score
    assert R.gaussian_selection_preselect(m, X, [3, 1], 5, mode)[0] == [1, 3]
    # position p carries preselect[p]: of the identical Gaussians 1 and 2 the larger INDEX comes first wherever it stands
    assert R.gaussian_selection_preselect(m, X, [2, 1, 0], 2, mode)[0] == [2, 1]
    assert R.gaussian_selection_preselect(m, X, [1, 0, 2], 2, mode)[0] == [2, 1]
    assert R.gaussian_selection_preselect(m, X, [4, 0, 3], 1, mode)[0] == [3]
    out, like, _ = R.gaussian_selection_preselect(m, X, [4], 3, mode)
    assert out == [4] and like == F32(-2)


def test_reference_mode_scores_a_range_when_first_and_last_index_say_so():
    """diag-gmm.cc:575: [3, 9, 5, 6] has back + 1 - front == 4, so the reference scores Gaussians 3, 4, 5, 6 for it; library
    mode scores 3, 9, 5, 6."""
    assert R.reference_scored([3, 9, 5, 6]).tolist() == [3, 4, 5, 6]
    assert R.reference_scored([3, 4, 5, 6]).tolist() == [3, 4, 5, 6]
    assert R.reference_scored([6, 5, 9, 3]).tolist() == [6, 5, 9, 3]
    assert R.reference_scored([7]).tolist() == [7]
    m = flat_model(np.arange(10.0))
    assert R.log_likelihoods_preselect(m, X, [3, 9, 5, 6], "reference").tolist() == [3, 4, 5, 6]
    assert R.log_likelihoods_preselect(m, X, [3, 9, 5, 6], "library").tolist() == [3, 9, 5, 6]


def test_nan_frame_has_no_selection():
    out, like, st = R.gaussian_selection_frame(random_model(0, 4, 2), np.asarray([np.nan, 1.0], F32), 2)
    assert out == [] and np.isnan(like) and st == 1


def test_contiguous_and_scattered_lists_give_the_same_posteriors_in_library_mode():
    """Gaussian 5 is a copy of Gaussian 4: the contiguous list [2, 3, 4] and the scattered [2, 3, 5] hold the same Gaussians in
    the same order, and library mode has one order of arithmetic for both - equal bits.  (The reference takes BLAS for the
    first and VecVec for the second.)"""
    m = random_model(3, 6, 7)
    for k in m:
        m[k][5] = m[k][4]
    feats = np.random.default_rng(4).standard_normal((9, 7)).astype(F32)
    a = R.global_acc_stats(m, feats, [[2, 3, 4]] * 9)
    b = R.global_acc_stats(m, feats, [[2, 3, 5]] * 9)
    assert np.array_equal(a["post"][:, [2, 3, 4]].view(np.int32), b["post"][:, [2, 3, 5]].view(np.int32))
    assert np.array_equal(a["frame_like"].view(np.int32), b["frame_like"].view(np.int32))
    assert not b["post"][:, 4].any() and not a["post"][:, 5].any()
    for t in range(9):
        assert np.array_equal(R.log_likelihoods_preselect(m, feats[t], [2, 3, 4]), R.log_likelihoods_preselect(m, feats[t])[2:5])


@pytest.mark.parametrize("mode", MODES)
def test_acc_loop_by_hand_and_weight_zero_skipped(mode):
    """Two equal Gaussians: posteriors 1/2 each times the weight; frame 1 has weight 0 and is skipped."""
    m = flat_model([0, 0])
    feats = np.asarray([[2.0], [100.0], [3.0]], F32)
    for gsel in (None, [[0, 1], [], [1, 0]]):
        r = R.global_acc_stats(m, feats, gsel, [1.0, 0.0, 2.0], 7, mode)
        assert r["used"].tolist() == [0, 2] and r["post"].tolist() == [[0.5, 0.5], [1.0, 1.0]]
        assert r["occ"].tolist() == [1.5, 1.5]
        assert r["mean_acc"].tolist() == [[0.5 * 2 + 1.0 * 3]] * 2 and r["var_acc"].tolist() == [[0.5 * 4 + 1.0 * 9]] * 2
        ln2 = F32(math.log(2.0))
        assert r["frame_like"].tolist() == [ln2, 0.0, ln2]
        assert r["file_weight"] == F32(3) and r["file_like"] == F32(ln2 + F32(F32(2) * ln2))
    r = R.global_acc_stats(m, feats, None, None, 5, mode)
    assert r["var_acc"] is None and r["occ"].tolist() == [1.5, 1.5] and r["mean_acc"].tolist() == [[52.5]] * 2


def test_both_branches_agree_when_every_gaussian_is_listed():
    m = random_model(5, 7, 3)
    feats = np.random.default_rng(6).standard_normal((11, 3)).astype(F32)
    a = R.global_acc_stats(m, feats, None, None)
    b = R.global_acc_stats(m, feats, [list(range(7))] * 11, None)
    for k in ("occ", "mean_acc", "var_acc", "post", "frame_like"):
        assert np.array_equal(a[k], b[k]), k


def test_matrix_form_sums_in_parts():
    """Under max_mem the utterance is one part; above it ceil(mem / max_mem) parts of ceil(T / parts) frames, the last shorter."""
    assert R.parts(100, 512) == [(0, 100)]
    assert R.parts(4882, 512) == [(0, 4882)]                       # 4882 * 512 * 4 = 9998336 <= 10000000
    assert R.parts(4883, 512) == [(0, 2442), (2442, 4883)]         # 10000384: two parts
    assert R.parts(5000, 2048) == [(0, 1000), (1000, 2000), (2000, 3000), (3000, 4000), (4000, 5000)]
    assert R.parts(2445, 2048) == [(0, 815), (815, 1630), (1630, 2445)]
    likes = np.asarray([1e8, 1.0, -1e8, 1.0], F32)
    assert R.sum_in_parts(likes, 4) == ((1e8 + 1.0) - 1e8) + 1.0
