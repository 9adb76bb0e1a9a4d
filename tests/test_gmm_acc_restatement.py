"""CPU: tests/gmm_acc_restatement.py on a case small enough to write the sums out, and the three accumulate binaries' loops
on the fMLLR end-to-end data: the routes agree where the reference's would, the totals are doubles summed in entry order, and
the restatement's own frame-order double sums are within the derived bound (gmm_acc_cases) of the exactly rounded sums."""
import numpy as np
import pytest

import gmm_acc_cases as C
import gmm_acc_restatement as A


def test_hand_case():
    """2 pdfs of 1 and 2 Gaussians, D = 2, 4 frames; every number is a dyadic fraction, so every sum is exact:
      frame 0  x = ( 1,    2   )  pdf 0: p = (1)
      frame 1  x = ( 3,   -1   )  pdf 1: p = (0.25, 0.75)
      frame 2  x = ( 0.5,  4   )  pdf 0: p = (0.5);  pdf 1: p = (0.5, 0.5)
      frame 3  x = (-2,    0.25)  pdf 1: p = (1, 0)"""
    off = np.array([0, 1, 3], np.int32)
    feats = np.array([[1, 2], [3, -1], [0.5, 4], [-2, 0.25]], np.float32)
    ent = C.entries([[0], [1], [0, 1], [1]], off)
    post = np.array([1.0, 0.25, 0.75, 0.5, 0.5, 0.5, 1.0, 0.0], np.float32)
    acc = A.accumulate_entries(A.init_accs(off, 2, "mvw"), feats, ent, post)
    assert acc["occ"].tolist() == [1.5, 1.75, 1.25]
    assert acc["mean_acc"].tolist() == [[1.25, 4.0], [-1.0, 2.0], [2.5, 1.25]]
    assert acc["var_acc"].tolist() == [[1.125, 12.0], [6.375, 8.3125], [6.875, 8.75]]
    assert acc["flags"] == 7 and acc["dim"] == 2
    mw = A.accumulate_entries(A.init_accs(off, 2, "mw"), feats, ent, post)
    assert mw["flags"] == 5 and mw["var_acc"] is None and mw["mean_acc"].tolist() == acc["mean_acc"].tolist()
    w = A.accumulate_entries(A.init_accs(off, 2, "w"), feats, ent, post)
    assert w["flags"] == 4 and w["mean_acc"] is None and w["var_acc"] is None and w["occ"].tolist() == acc["occ"].tolist()
    assert A.augment_flags("v") == 7 and A.augment_flags("") == 4 and A.augment_flags("m") == 5 and A.augment_flags("t") == 12
    assert A.augment_flags("mvwt") == 15 == A.augment_flags(A.kGmmAll) == A.augment_flags("a")        # the t bit stays: it is in the file


@pytest.fixture(scope="module")
def job(oracle):
    """Three utterances of the end-to-end case (820 frames), through the three loops once."""
    am, tid2pdf, utts = C.e2e_utterances(oracle)
    utts = utts[:3]
    post_route = A.acc_stats(am, tid2pdf, [(m, p) for _, m, p, _ in utts])
    ali_route = A.acc_stats_ali(am, tid2pdf, [(m, a) for _, m, _, a in utts])
    return dict(am=am, tid2pdf=tid2pdf, utts=utts, post=post_route, ali=ali_route)


def test_post_route(job):
    acc, tot_like, tot_t = job["post"]
    am, tid2pdf, utts = job["am"], job["tid2pdf"], job["utts"]
    # total_like / total_frames: doubles, entry by entry in order (mle-am-diag-gmm.cc:76-77), here from one stacked pass
    feats = np.concatenate([m for _, m, _, _ in utts])
    posts = [fr for _, _, p, _ in utts for fr in p]
    ent = A.R.entries_of(A.convert_posterior_to_pdfs(tid2pdf, posts), am["pdf_offsets"])
    gpost, like = A.R.component_posteriors(am, feats, ent)
    like_sum = frames_sum = 0.0
    for e in range(len(like)):
        like_sum += float(np.float32(like[e] * ent["weight"][e]))
        frames_sum += float(ent["weight"][e])
    assert acc["total_like"] == like_sum and acc["total_frames"] == frames_sum
    assert {0, 1, 2} <= set(np.diff(ent["feo"]).tolist())                  # frames without, with one and with two entries
    assert abs(acc["occ"].sum() - frames_sum) < 1e-3 and abs(tot_t - frames_sum) < 1e-2
    assert abs(tot_like - like_sum) < 1e-3 * abs(like_sum)
    # the transition accumulators: every (tid, weight) of the posteriors, in double
    want = np.zeros(len(tid2pdf))
    for fr in posts:
        for tid, w in fr:
            want[tid] += float(np.float32(w))
    assert np.array_equal(acc["transition_accs"], want) and want[0] == 0 and len(want) == 13
    # the restatement's own sums against the exactly rounded ones
    worst = C.check_bound(acc, am["pdf_offsets"], feats, ent, gpost, seed=1, label="restatement")
    print("restatement: worst error / bound", worst)
    # the stacked pass is the per-utterance loop: same entries in the same order
    stacked = A.accumulate_entries(A.init_accs(am["pdf_offsets"], feats.shape[1], "mvw"), feats, ent, gpost, like)
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.array_equal(stacked[k], acc[k]), k
    assert stacked["total_like"] == acc["total_like"]


def test_ali_route_is_the_post_route_of_its_alignment(job):
    acc, tot_like, tot_t = job["ali"]
    am, tid2pdf, utts = job["am"], job["tid2pdf"], job["utts"]
    via_post = A.acc_stats(am, tid2pdf, [(m, [[(int(t), 1.0)] for t in a]) for _, m, _, a in utts])[0]
    for k in ("occ", "mean_acc", "var_acc", "transition_accs"):
        assert np.array_equal(acc[k], via_post[k]), k
    assert acc["total_like"] == via_post["total_like"] and acc["total_frames"] == 820.0 and tot_t == 820
    assert acc["transition_accs"].sum() == 820.0
    assert abs(tot_like - acc["total_like"]) < 1e-3 * abs(tot_like)


def test_twofeats_and_flags(job):
    am, tid2pdf, utts = job["am"], job["tid2pdf"], job["utts"][:1]
    m, p = utts[0][1][:120], utts[0][2][:120]
    same = A.acc_stats(am, tid2pdf, [(m, m, p)], twofeats=True)[0]
    one = A.acc_stats(am, tid2pdf, [(m, p)])[0]
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.array_equal(same[k], one[k]), k                             # the second features = the first
    m2 = C.second_features(m, 9, 3)
    two = A.acc_stats(am, tid2pdf, [(m, m2, p)], twofeats=True)[0]
    assert two["dim"] == 9 and two["mean_acc"].shape == (28, 9) and np.array_equal(two["occ"], one["occ"])
    assert two["total_like"] == one["total_like"]
    mw = A.acc_stats(am, tid2pdf, [(m, p)], flags="mw")[0]
    assert mw["var_acc"] is None and np.array_equal(mw["mean_acc"], one["mean_acc"]) and mw["flags"] == 5
    # Init(am_gmm, kGmmAll) and StringToGmmFlags("mvwt"): the accumulators carry, and the file holds, 15
    assert one["flags"] == 15 and two["flags"] == 15 and job["ali"][0]["flags"] == 15 and job["post"][0]["flags"] == 15


def test_sum_accs_adds_the_files_floats_in_double(job):
    a, b = job["post"][0], job["ali"][0]
    s = A.sum_accs([a, b, a])
    assert s["occ"].dtype == np.float64
    assert np.array_equal(s["mean_acc"], (a["mean_acc"].astype(np.float32).astype(np.float64) + b["mean_acc"].astype(np.float32))
                          + a["mean_acc"].astype(np.float32))
    assert s["total_frames"] == a["total_frames"] + b["total_frames"] + a["total_frames"]
    assert np.array_equal(s["transition_accs"], a["transition_accs"] + b["transition_accs"] + a["transition_accs"])
