"""No GPU: tests/gselect_restatement.py in REFERENCE mode against what the reference's own compiled code produced
(tests/golden/gselect/reference_T200_G24_D5.npz: the inputs, and the lists of DiagGmm::GaussianSelection (n = 6) and
GaussianSelectionPreselect (n = 3 over those lists), the posteriors and the accumulators of gmm-global-acc-stats' gselect
loop, recorded from a program linked against the reference's objects).

THE NEAR-TIE SET.  The reference's score of a Gaussian is a float sum of 2 D + 1 terms in its BLAS's order; the restatement
accumulates in float64 and rounds once.  Either is within
    b = gamma_{D+2} (|g| + sum |x m| + 0.5 sum |x^2 v|),   gamma_k = k u / (1 - k u),  u = 2^-24
of the exact score (D products and D + 1 additions along any chain, the scaling by 0.5 exact).  Two scores whose float64
values are closer than b_i + b_j <= 2 max(b) may therefore compare differently on the two sides; where that happens among a
frame's top n + 1 the lists may differ.  The set of such frames is computed from the inputs alone, must hold at most 2 % of
the frames, and only outside it are the lists required to be equal.  (The seed of the committed inputs was picked on the CPU
so that the set is empty.)

WHAT THE REFERENCE SCORES FOR A LIST.  DiagGmm::LogLikelihoodsPreselect decides "contiguous range" from the list's first and last
index alone, and a list ordered by score that happens to satisfy back + 1 - front == size is scored as the RANGE front ...
front + size - 1 (gselect_restatement.reference_scored).  Frames of the recording do (frame 36 is one); reference mode restates
it and the recorded posteriors agree only with it restated.  The library scores the Gaussians a list names.

THE ACCUMULATORS.  Both sides sum the same lists.  A posterior is p_j = e^{f_j} / sum_k e^{f_k}; with every f within b of the
exact score on either side, the two sides' p differ by at most a factor e^{+-4 b}, and by the softmax's own float arithmetic,
(2 n + 10) u relative (tests/fmllr_cases.py: post_rel_bound).  Carried through the sums: sum_t dp |x|^k; plus each side's
summation, (T + 2) 2^-53 sum |t| against the exactly rounded sum (tests/gmm_acc_cases.py) - the restatement's own sums are held
to that against math.fsum here."""
import math
import os

import numpy as np
import pytest

import fmllr_cases as FC
import gselect_restatement as R
from conftest import GOLDEN

F32 = np.float32
U = 2.0 ** -24
PATH = os.path.join(GOLDEN, "gselect", "reference_T200_G24_D5.npz")


def score_bound(m, feats):
    """b [T, G]."""
    D = feats.shape[1]
    k = D + 2
    gamma = k * U / (1 - k * U)
    x = np.abs(feats.astype(np.float64))
    mag = np.abs(m["gconsts"].astype(np.float64))[None] + x @ np.abs(m["means_invvars"].astype(np.float64)).T \
        + 0.5 * (x * x) @ np.abs(m["inv_vars"].astype(np.float64)).T
    return gamma * mag


def exact_scores(m, feats, lists=None):
    x = feats.astype(np.float64)
    return m["gconsts"].astype(np.float64)[None] + x @ m["means_invvars"].astype(np.float64).T - 0.5 * (x * x) @ m["inv_vars"].astype(np.float64).T


def near_tie_frames(m, feats, n, lists=None):
    """Frames where two of the top n + 1 float64 scores (over all Gaussians, or over the frame's list) are closer than twice the
    bound."""
    s, b = exact_scores(m, feats), score_bound(m, feats)
    out = []
    for t in range(len(feats)):
        idx = np.arange(s.shape[1]) if lists is None else R.reference_scored(lists[t])        # what the reference scores
        top = np.sort(s[t, idx])[::-1][:n + 1]
        if len(top) > 1 and (-np.diff(top) < 2 * b[t, idx].max()).any():
            out.append(t)
    return out


@pytest.fixture(scope="module")
def rec():
    z = np.load(PATH)
    m = dict(gconsts=z["gconsts"], means_invvars=z["means_invvars"], inv_vars=z["inv_vars"])
    return z, m


def test_selection_lists_outside_the_near_tie_set(rec):
    z, m = rec
    feats, n, n2 = z["feats"], int(z["n"]), int(z["n2"])
    T = len(feats)
    assert (T, len(m["gconsts"]), feats.shape[1], n) == (200, 24, 5, 6)
    near = set(near_tie_frames(m, feats, n))
    print("near-tie frames:", sorted(near))
    assert len(near) <= 0.02 * T
    lists, like, status = R.gaussian_selection(m, feats, n, mode="reference")
    assert not status.any()
    for t in range(T):
        if t not in near:
            assert lists[t] == z["lists"][t].tolist(), t
    # the matrix form's double: the frames' float totals added in order (one part).  A total is a LogAdd chain over n scores:
    # the scores within 2 max(b) of each other on the two sides, each of the n steps rounding to float twice (the log1p term
    # and the sum) on either side - 4 n half-ulps of the total
    b = score_bound(m, feats).max(1)
    tol = float((2 * b + 4 * n * 0.5 * np.spacing(np.abs(like)).astype(np.float64)).sum())
    assert abs(R.sum_in_parts(like, 24) - float(z["ans"])) <= tol, (R.sum_in_parts(like, 24), float(z["ans"]), tol)
    # GaussianSelectionPreselect over the recorded lists
    near2 = set(near_tie_frames(m, feats, n2, z["lists"]))
    assert len(near2) <= 0.02 * T
    lists2, like2, _ = R.gaussian_selection(m, feats, n2, [v for v in z["lists"]], mode="reference")
    for t in range(T):
        if t not in near2:
            assert lists2[t] == z["lists2"][t].tolist(), t


def test_posteriors_and_accumulators(rec):
    z, m = rec
    feats, n = z["feats"], int(z["n"])
    T, D = feats.shape
    G = len(m["gconsts"])
    lists = [v for v in z["lists"]]
    r = R.global_acc_stats(m, feats, lists, None, 7, mode="reference")
    b = score_bound(m, feats)
    x = np.abs(feats.astype(np.float64))
    carried = dict(occ=np.zeros(G), mean_acc=np.zeros((G, D)), var_acc=np.zeros((G, D)))
    mag = dict(occ=np.zeros(G), mean_acc=np.zeros((G, D)), var_acc=np.zeros((G, D)))
    rec_post = z["post"].reshape(T, n)
    for t in range(T):
        ids = np.asarray(lists[t])
        p = r["post"][t, ids].astype(np.float64)
        rel = math.expm1(4 * b[t, R.reference_scored(ids)].max()) + 2 * float(FC.post_rel_bound(n))
        dp = rel * p + 2.0 ** -126
        assert (np.abs(rec_post[t].astype(np.float64) - p) <= dp).all(), t
        for k, xs in (("occ", None), ("mean_acc", x[t]), ("var_acc", x[t] * x[t])):
            carried[k][ids] += dp if xs is None else np.outer(dp, xs)
            mag[k][ids] += p if xs is None else np.outer(p, xs)
    worst = 0.0
    for k in ("occ", "mean_acc", "var_acc"):
        summation = (T + 2) * 2.0 ** -53 * mag[k]
        # the restatement's frame-order sums against the exactly rounded sums of its own addends
        for g in range(0, G, 5):
            for d in ([0] if k == "occ" else range(D)):
                terms = []
                for t in range(T):
                    if g in lists[t]:
                        p = float(r["post"][t, g])
                        xv = float(feats[t, d])
                        terms.append(p if k == "occ" else p * xv if k == "mean_acc" else p * (xv * xv))
                got = r[k][g] if k == "occ" else r[k][g, d]
                s = summation[g] if k == "occ" else summation[g, d]
                assert abs(got - math.fsum(terms)) <= s, (k, g, d)
        bound = 1.0001 * (carried[k] + 2 * summation * (1 + 2.0 ** -20))
        err = np.abs(z[k] - r[k])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), k
    print("accumulators: worst error / bound", worst)
    # file_like: a FLOAT running sum of the frames' likes on both sides.  A like is max + Log(sum): within 2 max(b) between the
    # sides plus (2 n + 3) half-ulps each (the sum's n adds, exp's and log's rounding, the final add); the running sum rounds
    # once per frame, relative to a partial sum of at most sum |like|, on each side
    like = np.abs(r["frame_like"].astype(np.float64))
    tol = float((2 * b.max(1) + 2 * (2 * n + 3) * 0.5 * np.spacing(np.abs(r["frame_like"])).astype(np.float64)).sum() + 2 * T * U * like.sum())
    assert abs(float(z["file_like"]) - float(r["file_like"])) <= tol, (float(z["file_like"]), float(r["file_like"]), tol)
