"""GPU: kh_gmm_preselect_posteriors and the accumulation of gmm-global-acc-stats (api.gmm_preselect_posteriors,
api.accumulate_global_gmm_stats) against the line-by-line restatement in library mode (tests/gselect_restatement.py).

The posteriors - one dense row per frame that is not skipped - and frame_like are bit-equal to the restatement.  The
accumulators are held three ways: to the bound tests/gmm_acc_cases.py derives, (n + 2) 2^-53 sum |t_e| against the exactly
rounded sums, as are the restatement's own frame-order sums; and bit-equal to api.gmm_acc_stats called by hand on the same
dense posteriors, which is what "the accumulation reuses kh_gmm_acc_stats unchanged" means."""
import numpy as np
import pytest
import torch

import gmm_acc_cases as AC
import gselect_cases as GC
import gselect_restatement as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def weights_for(seed, T):
    """Mostly 1, some fractions, zeros (skipped frames, -0.0 among them) and a negative one."""
    w = np.random.default_rng(seed).choice([1.0, 1.0, 1.0, 0.5, 0.25, 0.0], T).astype(F32)
    if T > 3:
        w[1], w[2], w[3] = 0.0, -0.5, -0.0
    return w


def one_pdf_entries(used, T, G):
    feo = np.zeros(T + 1, np.int64)
    feo[np.asarray(used, np.int64) + 1] = 1
    return dict(feo=np.cumsum(feo), pdf=np.zeros(len(used), np.int32), weight=np.ones(len(used), F32),
                goff=np.arange(len(used) + 1, dtype=np.int64) * G)


CASES = [  # G, D, T, list lengths, kind, stride, weights
    (5, 3, 40, [2], "unsorted", None, False),
    (5, 3, 40, [1, 5, 3], "scattered", 7, True),
    (70, 3, 300, [1, 64, 65, 6], "unsorted", None, True),
    (70, 40, 300, [6], "contiguous", 43, True),
    (600, 5, 20, [513, 3, 600], "unsorted", None, True),
    (2048, 40, 9, [5], "scattered", None, False),
]


@pytest.mark.parametrize("G,D,T,lengths,kind,stride,weighted", CASES)
def test_preselect_posteriors_and_accumulators(api, G, D, T, lengths, kind, stride, weighted):
    m = GC.model(G + D, G, D, [(0, 1)] if G > 1 else [])
    x, wide = GC.features(G + T, T, D, stride)
    gsel = GC.lists(G * 3 + T, T, G, lengths, kind)
    w = weights_for(T, T) if weighted else None
    gmm, feats = GC.device_model(api, m), GC.device_features(x, wide)
    want = R.global_acc_stats(m, x, gsel, w, 7)

    post, like, used = api.gmm_preselect_posteriors(gmm, feats, gsel, w)
    assert np.array_equal(used, want["used"]) and post.shape == (len(used), G)
    assert np.array_equal(post.cpu().numpy().view(np.int32), want["post"].view(np.int32))
    assert np.array_equal(like.view(np.int32), want["frame_like"].view(np.int32))
    assert api.gselect_last_timings()["used_frames"] == len(used)

    ent = one_pdf_entries(used, T, G)
    flat = want["post"].reshape(-1)
    for flags in ("w", "m", "mv", "mvw"):
        bits = api.gmm_flags(flags)
        got = api.accumulate_global_gmm_stats(gmm, feats, gsel, w, flags)
        assert got["flags"] == bits and got["dim"] == D
        assert (got["mean_acc"] is None) == (not bits & 1) and (got["var_acc"] is None) == (not bits & 2)
        by_hand = api.gmm_acc_stats(gmm, feats, ent, post.reshape(-1), bits)
        for k in ("occ", "mean_acc", "var_acc"):
            assert (got[k] is None and by_hand[k] is None) or np.array_equal(got[k], by_hand[k]), (flags, k)
        assert got["file_like"].dtype == np.float32 and got["file_like"] == want["file_like"] and got["file_weight"] == want["file_weight"]
        worst = AC.check_bound(got, [0, G], x, ent, flat, seed=G, label="device " + flags)
        print(flags, "worst error / bound: device", worst)
    ref = dict(occ=want["occ"], mean_acc=want["mean_acc"], var_acc=want["var_acc"])
    print("worst error / bound: restatement", AC.check_bound(ref, [0, G], x, ent, flat, seed=G, label="restatement"))


@pytest.mark.parametrize("G,D,T", [(5, 3, 40), (70, 40, 300)])
def test_no_gselect_branch_is_the_one_pdf_route(api, G, D, T):
    """gmm-global-acc-stats.cc:133-139, AccumulateFromDiag: kh_gmm_acc_component_posteriors + kh_gmm_acc_stats on the one-pdf
    model with the frame weights as entry weights - equal bits to that route called by hand, and the restatement's posteriors."""
    m = GC.model(G, G, D)
    x, wide = GC.features(T, T, D)
    w = weights_for(3, T)
    gmm, feats = GC.device_model(api, m), GC.device_features(x, wide)
    want = R.global_acc_stats(m, x, None, w, 7)
    got = api.accumulate_global_gmm_stats(gmm, feats, None, w, "mvw")
    used = np.nonzero(w != 0)[0]
    ent = one_pdf_entries(used, T, G)
    ent["weight"] = w[used]
    post, like = api.gmm_acc_component_posteriors(gmm, feats, ent)
    assert np.array_equal(post.cpu().numpy().view(np.int32), want["post"].reshape(-1).view(np.int32))
    assert np.array_equal(got["frame_like"][used].view(np.int32), like.cpu().numpy().view(np.int32))
    assert np.array_equal(got["frame_like"].view(np.int32), want["frame_like"].view(np.int32))
    by_hand = api.gmm_acc_stats(gmm, feats, ent, post, 7)
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.array_equal(got[k], by_hand[k]), k
    assert got["file_like"] == want["file_like"] and got["file_weight"] == want["file_weight"]
    AC.check_bound(got, [0, G], x, ent, want["post"].reshape(-1), seed=1, label="no gselect")
    # every Gaussian listed in order: the gselect branch computes the same posteriors
    full = api.accumulate_global_gmm_stats(gmm, feats, [np.arange(G)] * T, w, "mvw")
    for k in ("occ", "mean_acc", "var_acc", "frame_like"):
        assert np.array_equal(got[k], full[k]), k


def test_refusals_name_the_frame(api):
    m = GC.model(1, 6, 3)
    gmm = GC.device_model(api, m)
    feats = torch.zeros((4, 3), device="cuda")
    fn = "kh_gmm_preselect_posteriors: "

    def refused(gsel, w=None):
        with pytest.raises(api.KhError) as e:
            api.gmm_preselect_posteriors(gmm, feats, gsel, w)
        return str(e.value).split(": ", 1)[1]

    assert refused([[0], [1, 2, 1], [3], [4]]) == fn + "frame 1 lists Gaussian 1 twice"
    assert refused([[0], [1, 2], [], [4]]) == fn + "frame 2 has an empty list"
    assert refused([[0], [1, 2], [3], [6]]) == fn + "frame 3 lists Gaussian 6, the model has 6"
    assert refused([[0], [1, 2], [3], [-1]]) == fn + "frame 3 lists Gaussian -1, the model has 6"
    # a skipped frame's list is not looked at
    w = np.asarray([1, 0, 1, 1], F32)
    post, like, used = api.gmm_preselect_posteriors(gmm, feats, [[0], [1, 2, 1], [3], [4]], w)
    assert used.tolist() == [0, 2, 3] and like[1] == 0
    assert refused([[0], [], [3, 3], [4]], w) == fn + "frame 2 lists Gaussian 3 twice"
    with pytest.raises(api.KhError, match="frame 1 lists Gaussian 1 twice"):
        api.accumulate_global_gmm_stats(gmm, feats, [[0], [1, 2, 1], [3], [4]])
    with pytest.raises(api.KhError, match="3 lists for 4 frames"):
        api.gmm_preselect_posteriors(gmm, feats, [[0], [1], [2]])


def test_every_frame_skipped_and_no_frames(api):
    m = GC.model(2, 6, 3)
    gmm = GC.device_model(api, m)
    feats = torch.ones((3, 3), device="cuda")
    for gsel in (None, [[0], [1], [2]]):
        acc = api.accumulate_global_gmm_stats(gmm, feats, gsel, np.zeros(3, F32))
        assert not acc["occ"].any() and not acc["mean_acc"].any() and not acc["var_acc"].any()
        assert acc["file_like"] == 0 and acc["file_weight"] == 0 and acc["frame_like"].tolist() == [0, 0, 0]
    acc = api.accumulate_global_gmm_stats(gmm, torch.zeros((0, 3), device="cuda"), [])
    assert acc["occ"].shape == (6,) and not acc["occ"].any()


def test_same_bits_twice_and_into(api):
    m = GC.model(3, 70, 5)
    x, wide = GC.features(4, 300, 5)
    gsel = GC.lists(5, 300, 70, [6], "unsorted")
    gmm, feats = GC.device_model(api, m), GC.device_features(x, wide)
    a = api.accumulate_global_gmm_stats(gmm, feats, gsel)
    b = api.accumulate_global_gmm_stats(gmm, feats, gsel)
    for k in ("occ", "mean_acc", "var_acc", "frame_like"):
        assert np.array_equal(a[k], b[k]), k
    tot = api.accumulate_global_gmm_stats(gmm, feats[:100], gsel[:100])
    first = {k: tot[k].copy() for k in ("occ", "mean_acc", "var_acc")}
    second = api.accumulate_global_gmm_stats(gmm, feats[100:], gsel[100:])
    out = api.accumulate_global_gmm_stats(gmm, feats[100:], gsel[100:], into=tot)
    assert out is tot
    for k in first:
        assert np.array_equal(tot[k], first[k] + second[k]), k
    with pytest.raises(api.KhError, match="dimension or flags mismatch, 70, 5, mvw vs. 70, 5, 5"):
        api.accumulate_global_gmm_stats(gmm, feats, gsel, flags="m", into=tot)
