"""No GPU: tools/gselect_cpu_baseline.cc (the one-thread C++ statement the rate tool times) against
tests/gselect_restatement.py in library mode, bit for bit: lists, frame likelihoods, the posteriors over the selected lists,
their likelihoods, and the frame-order double sums - on the hand cases (ties between identical Gaussians, all scores equal,
n from 1 to above G) and on a random model, with and without a preselection."""
import importlib

import numpy as np
import pytest

import gselect_restatement as R

F32 = np.float32
RATE = importlib.import_module("tools.gselect_rate")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return RATE.cpu_baseline(str(tmp_path_factory.mktemp("gselect_baseline")), ["-Wall", "-Werror"])


def flat_model(gconsts, dim=1):
    g = np.asarray(gconsts, F32)
    return dict(gconsts=g, means_invvars=np.zeros((len(g), dim), F32), inv_vars=np.zeros((len(g), dim), F32))


def random_model(seed, G, D, same=()):
    rng = np.random.default_rng(seed)
    iv = rng.uniform(0.5, 2.0, (G, D)).astype(F32)
    m = dict(gconsts=rng.uniform(-8, -4, G).astype(F32), means_invvars=(rng.standard_normal((G, D)) * iv).astype(F32), inv_vars=iv)
    for a, b in same:
        for k in m:
            m[k][b] = m[k][a]
    return m


def compare(exe, tmp_path, m, feats, n, pre=None):
    got = RATE.run_cpu(exe, m, feats, n, str(tmp_path), pre)
    lists, like, status = R.gaussian_selection(m, feats, n, pre)
    assert not status.any()
    assert [v.tolist() for v in got["lists"]] == lists
    assert np.array_equal(got["frame_like"].view(np.int32), like.view(np.int32))
    acc = R.global_acc_stats(m, feats, lists, None, 7)
    for t in range(len(feats)):
        assert np.array_equal(got["post"][t].view(np.int32), acc["post"][t, lists[t]].view(np.int32)), t
    assert np.array_equal(got["post_like"].view(np.int32), acc["frame_like"].view(np.int32))
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.array_equal(got[k], acc[k]), k
    return got


HAND = [([1, 3, 3, 0], 2, [2, 1]), ([2, 2, 2, 2], 2, [3, 2]), ([5, 1, 5, 5], 2, [3, 2]), ([0.5, -1, 2, 1], 1, [2]),
        ([0.5, -1, 2, 1], 3, [2, 3, 0]), ([0.5, -1, 2, 1], 4, [2, 3, 0, 1]), ([0.5, -1, 2, 1], 7, [2, 3, 0, 1]), ([-7.25, -30], 1, [0])]


@pytest.mark.parametrize("gconsts,n,want", HAND)
def test_hand_cases(exe, tmp_path, gconsts, n, want):
    got = compare(exe, tmp_path, flat_model(gconsts), np.asarray([[0.75], [-2.0]], F32), n)
    assert got["lists"][0].tolist() == want and got["lists"][1].tolist() == want


def test_hand_preselection(exe, tmp_path):
    m = flat_model([0.5, 4, 4, 1, -2])
    feats = np.asarray([[0.75], [1.0], [2.0], [3.0]], F32)
    got = compare(exe, tmp_path, m, feats, 2, [[3, 1], [2, 1, 0], [1, 0, 2], [4]])
    assert [v.tolist() for v in got["lists"]] == [[1, 3], [2, 1], [2, 1], [4]]


@pytest.mark.parametrize("n", [1, 6, 70])
def test_random_model(exe, tmp_path, n):
    m = random_model(3, 70, 5, [(2, 3), (2, 67)])
    feats = np.random.default_rng(4).standard_normal((40, 5)).astype(F32)
    compare(exe, tmp_path, m, feats, n)
    rng = np.random.default_rng(5)
    pre = [rng.choice(70, int(rng.integers(1, 20)), replace=False) for _ in range(40)]
    compare(exe, tmp_path, m, feats, n, pre)
