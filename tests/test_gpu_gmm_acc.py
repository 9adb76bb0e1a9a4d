"""GPU: kh_gmm_acc_stats (csrc/kh_gmmacc.hip) and api.accumulate_gmm_stats against exactly rounded sums and against
tests/gmm_acc_restatement.py, with the bound tests/gmm_acc_cases.py derives.  Every test here fails on a library without the
kh_gmm_acc_* entry points."""
import numpy as np
import pytest
import torch

import fmllr_cases as FC
import gmm_acc_cases as C
import gmm_acc_restatement as A

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def sizes_model(api, off):
    """An api.AmDiagGmm that carries the pdf sizes only (all kh_gmm_acc_stats reads of the model)."""
    ng = int(off[-1])
    return api.AmDiagGmm(np.zeros(ng, np.float32), np.zeros((ng, 1), np.float32), np.ones((ng, 1), np.float32), off)


def model_of(api, am):
    return api.AmDiagGmm(am["gconsts"], am["means_invvars"], am["inv_vars"], am["pdf_offsets"])


def bits_equal(a, b):
    for k in ("occ", "mean_acc", "var_acc"):
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k


def raw_acc_stats(api, am, feats, ent, post, fill):
    """kh_gmm_acc_stats itself, with output buffers that hold `fill` before the call: the outputs are SET, not added to."""
    import ctypes
    from conftest import pkg
    capi = pkg("capi")
    T, D = int(feats.shape[0]), int(feats.shape[1])
    off = np.ascontiguousarray(am.pdf_offsets.cpu().numpy(), np.int32)
    ng = int(off[-1])
    occ, mean, var = np.full(ng, fill), np.full((ng, D), fill), np.full((ng, D), fill)
    feo, pdf, goff = (np.ascontiguousarray(ent[k], t) for k, t in (("feo", np.int64), ("pdf", np.int32), ("goff", np.int64)))
    ip, lp, dp = capi.c_int32_p, capi.c_int64_p, capi.c_double_p
    api.check(api.lib().kh_gmm_acc_stats(ctypes.c_void_p(feats.data_ptr()), T, D, max(int(feats.stride(0)), D), off.ctypes.data_as(ip),
                                         len(off) - 1, feo.ctypes.data_as(lp), pdf.ctypes.data_as(ip), goff.ctypes.data_as(lp),
                                         ctypes.c_void_p(post.data_ptr()), 7, occ.ctypes.data_as(dp), mean.ctypes.data_as(dp),
                                         var.ctypes.data_as(dp)))
    return dict(occ=occ, mean_acc=mean, var_acc=var)


def expected_groups(off, ent, C_cols, limit):
    """The group rule of csrc/kh_gmmacc_plan.h restated: consecutive pdfs while (chunks + 1) G C doubles per pdf fit the limit."""
    n = np.bincount(ent["pdf"], minlength=len(off) - 1)
    cost = [(-(-int(n[p]) // C.CHUNK) + 1) * int(off[p + 1] - off[p]) * C_cols * 8 for p in range(len(off) - 1)]
    groups, cur = 0, None
    for c in cost:
        if cur is None or cur + c > limit:
            groups, cur = groups + 1, c
        else:
            cur += c
    return groups


@pytest.mark.parametrize("dim", C.TILE_DIMS)
def test_tile_edges(api, dim):
    """Pdfs of 1, 2, 15, 16, 17, 33 Gaussians; 2 D + 1 = 3 ... 81 columns; 0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1 and
    2 chunk + 1 entries per pdf; frames of 0, 1 and 3 entries, two of one pdf in a frame; weights 0 and negative."""
    assert C.CHUNK == api.gmm_acc_chunk() and C.MAX_DIM == api.gmm_acc_max_dim() >= 120
    off, feats, ent, post = C.tile_case(dim, 200 + dim)
    am, x, p = sizes_model(api, off), dev(feats), dev(post)
    got = api.gmm_acc_stats(am, x, ent, p)
    assert got["occ"].dtype == np.float64 and got["mean_acc"].shape == (int(off[-1]), dim) == got["var_acc"].shape
    worst = C.check_bound(got, off, feats, ent, post, seed=dim, label="device D=%d" % dim)
    print("D", dim, "worst error / bound", worst)
    t = api.gmm_acc_last_timings()
    assert t["groups"] == 1 and t["chunks"] == 1 + 1 + 1 + 1 + 2 + 3 + 0 + 1 + 1
    assert t["workgroups"] == 1 + 1 + 1 + 1 + 2 * 2 + 3 * 3 + 0 + 1 + 1                 # chunks x 16-Gaussian row tiles
    empty = int(np.nonzero(np.asarray(C.TILE_COUNTS) == 0)[0][0])
    for k in ("occ", "mean_acc", "var_acc"):
        assert not got[k][off[empty]:off[empty + 1]].any()                              # a pdf no entry names
    # two calls: equal bits; and the library call SETS its outputs: buffers full of 7.5 come back the same, the pdf no entry
    # names as zeros
    bits_equal(api.gmm_acc_stats(am, x, ent, p), got)
    raw = raw_acc_stats(api, am, x, ent, p, 7.5)
    bits_equal(raw, got)
    assert not raw["occ"][off[empty]:off[empty + 1]].any() and not raw["var_acc"][off[empty]:off[empty + 1]].any()
    # flags: the same occ / mean_acc bits, None for the rest
    mw, w = api.gmm_acc_stats(am, x, ent, p, "mw"), api.gmm_acc_stats(am, x, ent, p, "w")
    assert mw["var_acc"] is None and w["var_acc"] is None and w["mean_acc"] is None
    bits_equal(dict(got, var_acc=None), mw)
    bits_equal(dict(got, var_acc=None, mean_acc=None), w)
    bits_equal(api.gmm_acc_stats(am, x, ent, p, "v"), got)                              # AugmentGmmFlags: v needs m and w
    # a strided feature tensor: equal bits
    wide = torch.zeros((feats.shape[0], dim + 3), device="cuda")
    wide[:, :dim] = x
    bits_equal(api.gmm_acc_stats(am, wide[:, :dim], ent, p), got)
    # a workspace that holds three partial tiles: many groups, the same bits
    cols = 2 * dim + 1
    limit = 3 * 16 * cols * 8
    api.gmm_acc_set_workspace_limit(limit)
    try:
        small = api.gmm_acc_stats(am, x, ent, p)
        t = api.gmm_acc_last_timings()
    finally:
        api.gmm_acc_set_workspace_limit(0)
    want_groups = expected_groups(off, ent, cols, limit)
    assert t["groups"] == want_groups >= 5 and t["chunks"] == 11
    bits_equal(small, got)


def test_max_dim_and_refusals(api):
    D = api.gmm_acc_max_dim()
    off, feats, ent, post = C.tile_case(D, 5, sizes=[17, 2, 1], counts=[C.CHUNK + 1, 3, 0])
    am = sizes_model(api, off)
    got = api.gmm_acc_stats(am, dev(feats), ent, dev(post))
    print("D", D, "worst error / bound", C.check_bound(got, off, feats, ent, post, seed=D, label="max dim"))
    wide = np.concatenate([feats, feats[:, :1]], axis=1)
    with pytest.raises(api.KhError, match="feature dimension %d, supported 1 ... %d" % (D + 1, D)):
        api.gmm_acc_stats(am, dev(wide), ent, dev(post))
    with pytest.raises(api.KhError, match="%d Gaussian posteriors for entries that hold %d" % (len(post) - 1, len(post))):
        api.gmm_acc_stats(am, dev(feats), ent, dev(post[:-1]))
    bad = dict(ent, pdf=ent["pdf"].copy())
    bad["pdf"][0] = 3
    with pytest.raises(api.KhError, match="entry 0 names pdf 3, the model has 3"):
        api.gmm_acc_stats(am, dev(feats), bad, dev(post))
    first = int(ent["pdf"][0])
    other = 1 if first != 1 else 0
    bad["pdf"][0] = other
    with pytest.raises(api.KhError, match="pdf %d has %d Gaussians in the model, entry 0 carries %d posteriors" %
                       (other, off[other + 1] - off[other], off[first + 1] - off[first])):
        api.gmm_acc_stats(am, dev(feats), bad, dev(post))
    bad = dict(ent, feo=ent["feo"].copy())
    bad["feo"][1] = bad["feo"][-1] + 5
    with pytest.raises(api.KhError, match="frame_entry_offsets runs backwards at frame 1"):
        api.gmm_acc_stats(am, dev(feats), bad, dev(post))


def test_no_frames_and_no_entries(api):
    off = np.array([0, 2, 5], np.int32)
    am = sizes_model(api, off)
    none = dict(feo=np.zeros(1, np.int64), pdf=np.zeros(0, np.int32), weight=np.zeros(0, np.float32), goff=np.zeros(1, np.int64))
    got = api.gmm_acc_stats(am, torch.zeros((0, 4), device="cuda"), none, torch.zeros(0, device="cuda"))
    assert got["occ"].tolist() == [0.0] * 5 and got["mean_acc"].shape == (5, 4) and not got["mean_acc"].any() and not got["var_acc"].any()
    # the library call itself, on buffers that are not zero before it: T = 0, and frames without entries
    for x, e in ((torch.zeros((0, 4), device="cuda"), none), (dev(np.ones((3, 4), np.float32)), C.entries([[], [], []], off))):
        raw = raw_acc_stats(api, am, x, e, torch.zeros(1, device="cuda"), -3.25)
        assert not raw["occ"].any() and not raw["mean_acc"].any() and not raw["var_acc"].any()
    ent = C.entries([[], [], []], off)
    got = api.gmm_acc_stats(am, dev(np.ones((3, 4), np.float32)), ent, torch.zeros(0, device="cuda"))
    assert not got["occ"].any() and not got["mean_acc"].any() and not got["var_acc"].any()
    assert api.gmm_acc_last_timings()["chunks"] == 0


# ---------------------------------------------------------------- the posteriors of the route
def test_acc_component_posteriors(api, oracle):
    """kh_gmm_acc_component_posteriors on the A1 case (pdfs of 1 ... 129 Gaussians, frames of 0, 1 and 3 entries, weights 0 and
    negative): within A1's bounds of the restatement, as kh_gmm_component_posteriors is; its exp and log are the float
    of the double function, as the restatement states them, so the count of posteriors that differ at all is printed (and is small against
    A1's); the same refusals."""
    am, feats, posts = FC.a1_case(oracle)
    ent = A.R.entries_of(posts, am["pdf_offsets"])
    want_post, want_like = A.R.component_posteriors(am, feats, ent)
    gmm = model_of(api, am)
    post, like = api.gmm_acc_component_posteriors(gmm, dev(feats), ent)
    post, like = post.cpu().numpy(), like.cpu().numpy()
    a1_post, a1_like = api.gmm_component_posteriors(gmm, dev(feats), ent)
    print("posteriors unequal to the restatement's:", int((post != want_post).sum()), "of", len(post), "(A1:",
          int((a1_post.cpu().numpy() != want_post).sum()), ") scores:", int((like != want_like).sum()), "of", len(like), "(A1:",
          int((a1_like.cpu().numpy() != want_like).sum()), ")")
    assert (np.abs(post.astype(np.float64) - want_post) <= FC.post_bound(want_post, ent["goff"])).all()
    assert (np.abs(like.astype(np.float64) - want_like) <= FC.like_bound(want_like, ent["goff"])).all()
    z = int(np.nonzero(ent["weight"] == 0)[0][0])
    assert (post[ent["goff"][z]:ent["goff"][z + 1]] == 0).all()
    wide = torch.zeros((feats.shape[0], feats.shape[1] + 3), device="cuda")
    wide[:, :feats.shape[1]] = dev(feats)
    post2, like2 = api.gmm_acc_component_posteriors(gmm, wide[:, :feats.shape[1]], ent)
    assert np.array_equal(post2.cpu().numpy().view(np.int32), post.view(np.int32)) and np.array_equal(like2.cpu().numpy(), like)
    bad = dict(ent, pdf=ent["pdf"].copy())
    bad["pdf"][0] = 1
    with pytest.raises(api.KhError, match="pdf 1 has 2 Gaussians"):
        api.gmm_acc_component_posteriors(gmm, dev(feats), bad)
    bad["pdf"][0] = 6
    with pytest.raises(api.KhError, match="names pdf 6"):
        api.gmm_acc_component_posteriors(gmm, dev(feats), bad)


# ---------------------------------------------------------------- the whole route: the posteriors, then the accumulation
@pytest.fixture(scope="module")
def routes(api, oracle):
    """Three routes, the device and the restatement once each: "post" - three utterances of the end-to-end case stacked (820
    frames, 13 dimensions); "two" - the same posteriors, the statistics from 9-dimensional second features; "ali" - an
    alignment (every weight 1) on a model with three pdfs of one Gaussian, 2 chunks + 40 frames."""
    am, tid2pdf, utts = C.e2e_utterances(oracle)
    utts = utts[:3]
    feats = np.concatenate([m for _, m, _, _ in utts])
    pdf_posts = A.convert_posterior_to_pdfs(tid2pdf, [fr for _, _, p, _ in utts for fr in p])
    out = dict(am=am, feats=feats, pdf_posts=pdf_posts)

    def route(name, am, feats, posts, feats2=None, **kw):
        x2 = feats if feats2 is None else feats2
        ref, ent, like, post = A.accumulate_for_gmm(A.init_accs(am["pdf_offsets"], x2.shape[1], "mvw"), am, feats, posts, feats2)
        got = api.accumulate_gmm_stats(model_of(api, am), dev(feats), stats_feats=None if feats2 is None else dev(feats2), **kw)
        out[name] = dict(got=got, ref=ref, ent=ent, like=like, post=post, am=am, feats=feats, stats_feats=x2)
    route("post", am, feats, pdf_posts, pdf_posts=pdf_posts)
    route("two", am, feats, pdf_posts, C.second_features(feats, 9, 3), pdf_posts=pdf_posts)
    am1 = FC.model([1, 1, 3, 1], 13, 71, oracle)
    rng = np.random.default_rng(72)
    T = 2 * C.CHUNK + 40
    feats1 = FC.scaled_frames(rng, T, 13)
    tid2pdf1 = np.array([-1, 0, 0, 1, 2, 3, 3], np.int32)
    ali = rng.integers(1, 7, T)
    route("ali", am1, feats1, [[(int(tid2pdf1[t]), 1.0)] for t in ali], alignments=ali, tid2pdf=tid2pdf1)
    out["ali"]["alignment"] = ali
    return out


def check_route(r, label):
    """The device route against the restatement: the accumulators within the A1 bound carried through the sums, total_frames
    equal, total_like within the sum of the entries' like_bound (and the float product's rounding on each side)."""
    got, ref, ent, like = r["got"], r["ref"], r["ent"], r["like"]
    C.check_carried(got, ref, C.carried_bound(r["am"]["pdf_offsets"], r["stats_feats"], ent, r["post"]), label)
    assert got["total_frames"] == ref["total_frames"]
    tol = float((FC.like_bound(like, ent["goff"]) * np.abs(ent["weight"].astype(np.float64))).sum())
    tol += float(np.abs(np.spacing((like * ent["weight"]).astype(np.float32))).sum())
    print(label, "total_like", got["total_like"], "reference", ref["total_like"], "tolerance", tol)
    assert abs(got["total_like"] - ref["total_like"]) <= tol


def test_accumulate_gmm_stats(api, routes):
    am, feats, pdf_posts = routes["am"], routes["feats"], routes["pdf_posts"]
    got = routes["post"]["got"]
    assert got["dim"] == 13 and got["flags"] == 7 and got["pdf_offsets"].tolist() == list(am["pdf_offsets"])
    check_route(routes["post"], "post route")
    # the device's own sums against the exactly rounded ones, on the device's own posteriors
    gmm, x = model_of(api, am), dev(feats)
    ent = api.fmllr_entries(pdf_posts, am["pdf_offsets"])
    post, _ = api.gmm_acc_component_posteriors(gmm, x, ent)
    print("worst error / bound", C.check_bound(got, am["pdf_offsets"], feats, ent, post.cpu().numpy(), seed=9, label="route"))
    # into: the sum of two separate calls, in double
    half = 400
    a = api.accumulate_gmm_stats(gmm, x[:half], pdf_posts=pdf_posts[:half])
    b = api.accumulate_gmm_stats(gmm, x[half:], pdf_posts=pdf_posts[half:])
    want = {k: a[k] + b[k] for k in ("occ", "mean_acc", "var_acc", "total_like", "total_frames")}
    acc = api.accumulate_gmm_stats(gmm, x[:half], pdf_posts=pdf_posts[:half])
    out = api.accumulate_gmm_stats(gmm, x[half:], pdf_posts=pdf_posts[half:], into=acc)
    assert out is acc
    bits_equal(acc, want)
    assert acc["total_like"] == want["total_like"] and acc["total_frames"] == want["total_frames"]
    with pytest.raises(api.KhError, match="dimension or flags mismatch"):
        api.accumulate_gmm_stats(gmm, x[:half], pdf_posts=pdf_posts[:half], flags="mw", into=acc)
    # the flags an accumulator carries are the file's: the binaries' kGmmAll / "mvwt" keep the transition bit, the sums are the same
    full, ent2, like2 = api.accumulate_gmm_stats(gmm, x, pdf_posts=pdf_posts, flags="mvwt", return_entries=True)
    assert full["flags"] == 15 == api.gmm_flags(api.kGmmAll) and api.gmm_flags("mw") == 5 and api.gmm_flags("") == 4
    bits_equal(full, got)
    assert len(like2) == len(ent2["pdf"]) == len(routes["post"]["like"]) and full["total_like"] == got["total_like"]
    with pytest.raises(api.KhError, match="dimension or flags mismatch, 3, 13, mvw vs. 3, 13, 15"):
        api.accumulate_gmm_stats(gmm, x[:half], pdf_posts=pdf_posts[:half], flags="mvwt", into=acc)


def test_two_feature_route(api, routes):
    """D1 = 13 for the posteriors, D2 = 9 for the statistics."""
    r = routes["two"]
    assert np.array_equal(r["like"], routes["post"]["like"])
    assert r["got"]["dim"] == 9 and r["got"]["mean_acc"].shape == (28, 9)
    check_route(r, "two features")
    assert np.array_equal(r["got"]["occ"], routes["post"]["got"]["occ"]) and r["got"]["total_like"] == routes["post"]["got"]["total_like"]
    with pytest.raises(api.KhError, match="mismatched numbers of frames 820 vs. 819"):
        api.accumulate_gmm_stats(model_of(api, r["am"]), dev(r["feats"]), pdf_posts=routes["pdf_posts"], stats_feats=dev(r["stats_feats"][:-1]))


def test_alignments_on_single_gaussian_pdfs_are_exact(routes):
    """Every weight 1 on pdfs of one Gaussian: the posterior is 1 and occ is a count, bit-equal to the restatement's."""
    r = routes["ali"]
    got, ref, ali = r["got"], r["ref"], r["alignment"]
    single = [0, 1, 5]                                                  # the Gaussians of the one-Gaussian pdfs
    assert np.array_equal(got["occ"][single], ref["occ"][single])
    assert got["occ"][single].tolist() == [float(np.isin(ali, (1, 2)).sum()), float((ali == 3).sum()), float(np.isin(ali, (5, 6)).sum())]
    assert got["total_frames"] == float(len(ali))
    check_route(r, "alignments")


def test_written_floats_equal_or_adjacent(routes):
    """As written to a file (floats), the device route and the restatement agree elementwise to equal or adjacent floats; the
    count of unequal elements is printed.  This is what kh_gmm_acc_component_posteriors is for: with stage A1's posteriors
    (the device library's expf, up to 3 float ulps from the restatement's) mean_acc elements whose addends cancel
    (sum |t| / |sum t| of 76 - 146) differed by 2 - 4 float ulps on these routes."""
    for name in ("post", "two", "ali"):
        C.compare_written(A.as_written(routes[name]["got"]), A.as_written(routes[name]["ref"]), name)
