"""GPU: kh_mllt_acc_stats (csrc/kh_mllt.hip) and api.accumulate_mllt_stats against exactly rounded sums of exactly made
operands and against tests/mllt_restatement.py, with the bound tests/mllt_cases.py derives:
    |got - exact| <= (n + 2) 2^-53 sum |t_i|,   t_i = w_i[j] o_i[a] o_i[b]  as rationals.
Worst error / bound reached on an MI355X: printed by every test; recorded in DESIGN.md.
Every test here fails on a library without the kh_mllt_* entry points."""
import ctypes

import numpy as np
import pytest
import torch

import fmllr_cases as FC
import mllt_cases as C
import mllt_restatement as M

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def model_of(api, c):
    ng = int(c["off"][-1])
    return api.AmDiagGmm(np.zeros(ng, np.float32), c["mi"], c["iv"], c["off"])


def raw_acc_stats(api, am, feats, ent, post, fill):
    """kh_mllt_acc_stats itself, with an output buffer that holds `fill` before the call: the output is SET, not added to."""
    from conftest import pkg
    capi = pkg("capi")
    T, D = int(feats.shape[0]), int(feats.shape[1])
    off = np.ascontiguousarray(am.pdf_offsets.cpu().numpy(), np.int32)
    G = np.full((D, D * (D + 1) // 2), fill)
    feo, pdf, goff = (np.ascontiguousarray(ent[k], t) for k, t in (("feo", np.int64), ("pdf", np.int32), ("goff", np.int64)))
    ip, lp = capi.c_int32_p, capi.c_int64_p
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    api.check(api.lib().kh_mllt_acc_stats(p(feats), T, D, max(int(feats.stride(0)), D), p(am.means_invvars), p(am.inv_vars),
                                          off.ctypes.data_as(ip), len(off) - 1, feo.ctypes.data_as(lp), pdf.ctypes.data_as(ip),
                                          goff.ctypes.data_as(lp), p(post), G.ctypes.data_as(capi.c_double_p)))
    return G


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def run_case(api, dim, n, seed):
    c = C.kernel_case(dim, n, seed)
    am, x, p = model_of(api, c), dev(c["feats"]), dev(c["post"])
    G = api.mllt_acc_stats(am, x, c["ent"], p)
    assert G.dtype == np.float64 and G.shape == (dim, dim * (dim + 1) // 2)
    t = api.mllt_last_timings()
    slice_len, slices, wgs = C.slice_plan(n, dim)
    assert (t["items"], t["slices"], t["workgroups"]) == (n, slices, wgs), (t, n, dim)
    o, w, _ = C.items_of(c["off"], c["mi"], c["iv"], c["feats"], c["ent"], c["post"])
    assert len(o) == n
    worst = C.check_bound(G, o, w, dim, seed, "device D=%d n=%d" % (dim, n))
    return c, am, x, p, G, worst


@pytest.mark.parametrize("dim", C.DIMS)
def test_tile_edges(api, dim):
    """D = 1 ... kh_mllt_max_dim: Q = 1 ... 2080 columns (Q = 496 at D = 31 is a whole number of tiles), 1 ... 4 row tiles;
    0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1 and 2 chunk + 1 items; pdfs of 1, 2, 16, 17 Gaussians; frames of 0, 1 and 3
    entries; posteriors 0 and negative."""
    assert (C.CHUNK, C.MAX_SLICES, C.MAX_DIM) == (api.mllt_chunk(), api.mllt_max_slices(), api.mllt_max_dim()) and C.MAX_DIM >= 64
    worst = 0.0
    for n in C.ITEM_COUNTS:
        c, am, x, p, G, wr = run_case(api, dim, n, 1000 * dim + n)
        worst = max(worst, wr)
        if n == 0:
            assert not G.any()
    print("D", dim, "worst error / bound", worst)
    # the last case (2 chunks + 1 items, 3 slices): two calls give equal bits; the library call SETS its output
    assert bits_equal(api.mllt_acc_stats(am, x, c["ent"], p), G)
    assert bits_equal(raw_acc_stats(api, am, x, c["ent"], p, 7.5), G)
    # a strided feature tensor: equal bits
    wide = torch.zeros((c["feats"].shape[0], dim + 3), device="cuda")
    wide[:, :dim] = x
    assert bits_equal(api.mllt_acc_stats(am, wide[:, :dim], c["ent"], p), G)
    # no items: a buffer full of 7.5 comes back as zeros
    assert not raw_acc_stats(api, am, x, c["ent"], torch.zeros_like(p), 7.5).any()


def test_slice_length_grows(api):
    """D = 2, max_slices chunk + 1 items: the first size at which a slice is two chunks long."""
    n = C.MAX_SLICES * C.CHUNK + 1
    c, am, x, p, G, worst = run_case(api, 2, n, 77)
    assert C.slice_plan(n, 2)[0] == 2 * C.CHUNK and api.mllt_last_timings()["slices"] == C.MAX_SLICES // 2 + 1
    print("D 2 n", n, "worst error / bound", worst)


def test_refusals_leave_the_library_working(api):
    D = api.mllt_max_dim()
    c = C.kernel_case(D + 1, 5, 3)
    with pytest.raises(api.KhError, match="feature dimension %d, supported 1 ... %d" % (D + 1, D)):
        api.mllt_acc_stats(model_of(api, c), dev(c["feats"]), c["ent"], dev(c["post"]))
    c = C.kernel_case(5, 40, 4)
    am, x, p = model_of(api, c), dev(c["feats"]), dev(c["post"])
    ent = c["ent"]
    bad = dict(ent, pdf=ent["pdf"].copy())
    bad["pdf"][0] = 4
    with pytest.raises(api.KhError, match="entry 0 names pdf 4, the model has 4"):
        api.mllt_acc_stats(am, x, bad, p)
    bad["pdf"][0] = 0                                                    # entry 0 is of pdf 3 (17 Gaussians)
    with pytest.raises(api.KhError, match="pdf 0 has 1 Gaussians in the model, entry 0 carries 17 posteriors"):
        api.mllt_acc_stats(am, x, bad, p)
    bad = dict(ent, feo=ent["feo"].copy())
    bad["feo"][1] = bad["feo"][-1] + 5
    with pytest.raises(api.KhError, match="frame_entry_offsets runs backwards at frame 1"):
        api.mllt_acc_stats(am, x, bad, p)
    with pytest.raises(api.KhError, match="%d Gaussian posteriors for entries that hold %d" % (len(c["post"]) - 1, len(c["post"]))):
        api.mllt_acc_stats(am, x, ent, p[:-1])
    G = api.mllt_acc_stats(am, x, ent, p)                               # the next call works
    o, w, _ = C.items_of(c["off"], c["mi"], c["iv"], c["feats"], ent, c["post"])
    C.check_bound(G, o, w, 5, 4, "after refusals")


def test_no_frames_and_no_entries(api):
    c = C.kernel_case(4, 0, 9)
    am = model_of(api, c)
    none = dict(feo=np.zeros(1, np.int64), pdf=np.zeros(0, np.int32), weight=np.zeros(0, np.float32), goff=np.zeros(1, np.int64))
    G = raw_acc_stats(api, am, torch.zeros((0, 4), device="cuda"), none, torch.zeros(1, device="cuda"), -3.25)
    assert G.shape == (4, 10) and not G.any()
    ent = dict(feo=np.zeros(4, np.int64), pdf=np.zeros(0, np.int32), weight=np.zeros(0, np.float32), goff=np.zeros(1, np.int64))
    assert not api.mllt_acc_stats(am, dev(np.ones((3, 4), np.float32)), ent, torch.zeros(0, device="cuda")).any()
    assert api.mllt_last_timings()["items"] == 0
    acc = api.accumulate_mllt_stats(am, dev(np.ones((3, 4), np.float32)), [[], [], []])
    assert acc["beta"] == 0.0 and acc["dim"] == 4 and not acc["G"].any()


def test_separates_posteriors(api, oracle):
    """The device's own posteriors fed to the restatement's pruning and sums agree with api.accumulate_mllt_stats within the
    summation bound alone: the same draws (kh_rand_prune against the restatement's RandPrune after the same srand), hence
    the same items; beta bit for bit.  At rand_prune 0.25 and 0 (no draw), and at 4.0 where every survivor is +-4."""
    am = FC.model([1, 2, 16, 17, 5], 13, 41, oracle)
    rng = np.random.default_rng(42)
    T = 150
    feats = FC.scaled_frames(rng, T, 13)
    posts = []
    for t in range(T):
        k = int(rng.choice([0, 1, 1, 1, 3]))
        posts.append([(int(p), float(w)) for p, w in zip(sorted(rng.choice(5, k, replace=False)), rng.choice([1.0, 0.5, 0.25, -0.5], k))])
    gmm = api.AmDiagGmm(am["gconsts"], am["means_invvars"], am["inv_vars"], am["pdf_offsets"])
    x = dev(feats)
    ent = api.fmllr_entries(posts, am["pdf_offsets"])
    post, _ = api.gmm_acc_component_posteriors(gmm, x, ent)
    post = post.cpu().numpy()
    for prune in (0.25, 0.0, 4.0):
        got, ent2, like = api.accumulate_mllt_stats(gmm, x, posts, rand_prune=prune, seed=11, return_entries=True)
        assert np.array_equal(ent2["goff"], ent["goff"]) and len(like) == len(ent["pdf"])
        M.srand(11)
        before = M.DRAWS[0]
        ref = M.accumulate_entries(M.init_accs(13, prune), am, feats, ent, post)
        draws = M.DRAWS[0] - before
        assert (draws == 0) == (prune == 0.0)
        assert got["beta"] == ref["beta"] and got["dim"] == 13
        M.srand(11)
        pruned = np.array([M.rand_prune(v, prune) for v in post], np.float32)      # the same draws once more: the items
        o, w, p = C.items_of(am["pdf_offsets"], am["means_invvars"], am["inv_vars"], feats, ent, pruned)
        if prune == 4.0:
            assert set(np.abs(p).tolist()) <= {4.0}
        print("rand_prune", prune, "items", len(p), "of", int((post != 0).sum()), "draws", draws,
              "device worst error / bound", C.check_bound(got["G"], o, w, 13, 5, "device"),
              "restatement", C.check_bound(ref["G"], o, w, 13, 5, "restatement"))
        assert api.mllt_last_timings()["items"] == len(p)
    # into: the sum of two calls, in double; dims must agree
    a = api.accumulate_mllt_stats(gmm, x[:70], posts[:70], rand_prune=0.0)
    b = api.accumulate_mllt_stats(gmm, x[70:], posts[70:], rand_prune=0.0)
    acc = api.accumulate_mllt_stats(gmm, x[:70], posts[:70], rand_prune=0.0)
    out = api.accumulate_mllt_stats(gmm, x[70:], posts[70:], rand_prune=0.0, into=acc)
    assert out is acc and bits_equal(acc["G"], a["G"] + b["G"])
    assert acc["beta"] == api.accumulate_mllt_stats(gmm, x, posts, rand_prune=0.0)["beta"]      # beta runs on, entry by entry
    assert abs(acc["beta"] - (a["beta"] + b["beta"])) <= 2.0 ** -50 * abs(acc["beta"])
    with pytest.raises(api.KhError, match="summing accs of different size"):
        api.accumulate_mllt_stats(gmm, x, posts, into=dict(beta=0.0, G=np.zeros((3, 6)), dim=3))
    # segments: the accumulation per utterance, the utterances added in order - the same bits however they are grouped into calls
    whole = api.accumulate_mllt_stats(gmm, x, posts, rand_prune=0.25, seed=1, segments=[0, 40, 70, 70, 150])
    part = api.accumulate_mllt_stats(gmm, x[:70], posts[:70], rand_prune=0.25, seed=1, segments=[0, 40, 70])
    part = api.accumulate_mllt_stats(gmm, x[70:], posts[70:], rand_prune=0.25, seed=1, segments=[0, 0, 80], into=part)
    assert bits_equal(whole["G"], part["G"]) and whole["beta"] == part["beta"] and whole["draws"] == part["draws"] > 0
    one = api.accumulate_mllt_stats(gmm, x, posts, rand_prune=0.25, seed=1)
    assert one["beta"] == whole["beta"] and one["draws"] == whole["draws"] and np.allclose(one["G"], whole["G"], rtol=1e-9, atol=1e-9)
    with pytest.raises(api.KhError, match="segments must run from 0 to 150"):
        api.accumulate_mllt_stats(gmm, x, posts, segments=[0, 149])
