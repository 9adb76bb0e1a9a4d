"""GPU: kh_lda_acc_stats (csrc/kh_lda.hip) and api.accumulate_lda_stats against exactly rounded sums of exactly made operands
and against tests/lda_restatement.py, with the bound tests/lda_cases.py derives:
    |got - exact| <= (n + 2) 2^-53 sum |t_i|,
t_i = (w_i x_i[a]) x_i[b] over all items for `second`, w_i x_i[d] and w_i over the class's items for `first` and `zero`, as
rationals wherever D <= 5.  Every element is checked where D <= 5; above, sampled elements with the last packed element, a
diagonal-tile and an off-diagonal-tile element and the last row of `first` (lda_cases.second_picks, first_picks).
`zero` is additionally bit-equal to the restatement: the weights of the cases are multiples of 2^-10 with a sum below 2^40,
so every order of adding them is exact (lda_cases.zero_is_exact, asserted).
Worst error / bound reached on an MI355X: printed by every test; recorded in DESIGN.md.
Every test here fails on a library without the kh_lda_* entry points."""
import ctypes

import numpy as np
import pytest
import torch

import lda_cases as C
import mllt_restatement as M

pytestmark = pytest.mark.gpu
KEYS = ("zero", "first", "second")


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def raw_acc_stats(api, feats, ent, num_classes, fill, add, segments=None):
    """kh_lda_acc_stats itself, with output buffers that hold `fill` before the call."""
    from conftest import pkg
    capi = pkg("capi")
    T, D = int(feats.shape[0]), int(feats.shape[1])
    out = dict(zero=np.full(num_classes, fill), first=np.full((num_classes, D), fill), second=np.full(D * (D + 1) // 2, fill))
    feo, pdf, w = (np.ascontiguousarray(ent[k], t) for k, t in (("feo", np.int64), ("pdf", np.int32), ("weight", np.float32)))
    seg = np.ascontiguousarray([0, T] if segments is None else segments, np.int64)
    dp, lp = capi.c_double_p, capi.c_int64_p
    api.check(api.lib().kh_lda_acc_stats(ctypes.c_void_p(feats.data_ptr()), T, D, max(int(feats.stride(0)), D), feo.ctypes.data_as(lp),
                                         pdf.ctypes.data_as(capi.c_int32_p), w.ctypes.data_as(capi.c_float_p), num_classes,
                                         seg.ctypes.data_as(lp), len(seg) - 1, add, out["zero"].ctypes.data_as(dp),
                                         out["first"].ctypes.data_as(dp), out["second"].ctypes.data_as(dp)))
    return out


def bits_equal(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in KEYS)


def check(api, c, acc, seed, label, segments=None, limit=C.DEFAULT_LIMIT):
    """Shapes, the plan counters, the bound, and the counts bit for bit.  Returns the worst error / bound."""
    dim, nc = c["feats"].shape[1], c["num_classes"]
    x, w, cls = C.items_of(c["feats"], c["ent"])
    assert acc["zero"].shape == (nc,) and acc["first"].shape == (nc, dim) and acc["second"].shape == (dim * (dim + 1) // 2,)
    assert all(acc[k].dtype == np.float64 for k in KEYS) and (acc["dim"], acc["num_classes"]) == (dim, nc)
    t = api.lda_last_timings()
    seg_items = C.segment_items(c["ent"], [0, len(c["feats"])] if segments is None else segments)
    assert (t["items"], t["slices"], t["workgroups"], t["passes"]) == (len(w),) + C.plan(seg_items, dim, limit), (t, label)
    worst = C.check_bound(acc, x, w, cls, seed, label)
    assert C.zero_is_exact(w) and np.array_equal(acc["zero"], C.restate_zero(c["ent"], nc))
    if len(w) == 0:
        assert not any(acc[k].any() for k in KEYS)
    return worst


@pytest.mark.parametrize("dim", C.DIMS)
def test_tile_edges(api, dim):
    """D = 1 ... kh_lda_max_dim: one tile; a diagonal tile with a ragged edge (15, 17 ...); 3 tile pairs (17 ... 32) and 6
    (33); 36 pairs in 3 pairs of super tiles, the diagonal ones with their idle upper tiles (117); the limit (512: 36 pairs
    of super tiles).  0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1 and 2 chunk + 1 items; frames of 0, 1 and 3 entries, two
    entries of one frame on different pdfs, a class without items; weights 0, -0.0 and negative."""
    assert (C.CHUNK, C.MAX_SLICES, C.MAX_DIM) == (api.lda_chunk(), api.lda_max_slices(), api.lda_max_dim()) and C.MAX_DIM >= 512
    worst = 0.0
    for n in C.ITEM_COUNTS:
        c = C.kernel_case(dim, n, 1000 * dim + n)
        x = dev(c["feats"])
        acc = api.lda_acc_stats(x, c["ent"], c["num_classes"])
        worst = max(worst, check(api, c, acc, dim + n, "device D=%d n=%d" % (dim, n)))
    print("D", dim, "worst error / bound", worst)
    # the last case (2 chunks + 1 items, 3 slices): two calls give equal bits; a buffer of 7.5 comes back SET
    ent, nc = c["ent"], c["num_classes"]
    assert bits_equal(api.lda_acc_stats(x, ent, nc), acc)
    assert bits_equal(raw_acc_stats(api, x, ent, nc, 7.5, 0), acc)
    # under add it comes back 7.5 plus the sum: one addition onto what the buffer held; a class without items keeps 7.5
    added = raw_acc_stats(api, x, ent, nc, 7.5, 1)
    x_, w_, cls_ = C.items_of(c["feats"], ent)
    has = np.isin(np.arange(nc), cls_)
    assert not has[C.EMPTY_CLASS] and has.sum() == nc - 1
    assert np.array_equal(added["second"], 7.5 + acc["second"])
    assert np.array_equal(added["first"], np.where(has[:, None], 7.5 + acc["first"], 7.5))
    assert np.array_equal(added["zero"], np.where(has, 7.5 + acc["zero"], 7.5))
    # a strided feature tensor: equal bits
    wide = torch.zeros((c["feats"].shape[0], dim + 3), device="cuda")
    wide[:, :dim] = x
    assert bits_equal(api.lda_acc_stats(wide[:, :dim], ent, nc), acc)
    # no item: a buffer full of 7.5 comes back as zeros, or unchanged under add
    none = dict(ent, weight=np.where(np.arange(len(ent["pdf"])) % 2, np.float32(-0.0), np.float32(0.0)).astype(np.float32))
    assert not any(raw_acc_stats(api, x, none, nc, 7.5, 0)[k].any() for k in KEYS)
    assert all((raw_acc_stats(api, x, none, nc, 7.5, 1)[k] == 7.5).all() for k in KEYS)
    assert api.lda_last_timings()["items"] == 0


def test_slice_length_grows(api):
    """D = 2, max_slices chunk + 1 items in one segment: the first size at which a slice is two chunks long."""
    n = C.MAX_SLICES * C.CHUNK + 1
    c = C.big_case(2, n, 77)
    acc = api.lda_acc_stats(dev(c["feats"]), c["ent"], c["num_classes"])
    assert C.slice_len(n) == 2 * C.CHUNK and C.slice_len(n - 1) == C.CHUNK and api.lda_last_timings()["slices"] == C.MAX_SLICES // 2 + 1
    print("D 2 n", n, "worst error / bound", check(api, c, acc, 3, "slice growth"))


def test_repeatability_and_workspace_cap(api):
    """Segments of 2 chunk + 1, 0, 5 and chunk + 1 items: 3 + 1 + 2 slices.  A workspace limit of two slices' partial sums
    makes 3 passes, one of them ending inside a segment; of one slice's, 6 passes.  Equal bits throughout.  A limit one byte
    below a slice's partial sums is refused naming the bytes, before any launch, and the next call works."""
    dim = 33
    parts = [C.kernel_case(dim, n, 50 + n) for n in (2 * C.CHUNK + 1, 0, 5, C.CHUNK + 1)]
    feats = np.concatenate([p["feats"] for p in parts])
    segments = np.cumsum([0] + [len(p["feats"]) for p in parts])
    off = np.cumsum([0] + [len(p["ent"]["pdf"]) for p in parts])
    ent = dict(feo=np.concatenate([[0]] + [p["ent"]["feo"][1:] + o for p, o in zip(parts, off)]).astype(np.int64),
               pdf=np.concatenate([p["ent"]["pdf"] for p in parts]), weight=np.concatenate([p["ent"]["weight"] for p in parts]))
    c = dict(feats=feats, ent=ent, num_classes=C.NUM_CLASSES)
    x = dev(feats)
    acc = api.lda_acc_stats(x, ent, C.NUM_CLASSES, segments=segments)
    assert api.lda_last_timings()["slices"] == 6 and api.lda_last_timings()["passes"] == 1
    print("segments worst error / bound", check(api, c, acc, 9, "segments", segments))
    assert bits_equal(api.lda_acc_stats(x, ent, C.NUM_CLASSES, segments=segments), acc)
    slice_bytes = 8 * dim * (dim + 1) // 2
    try:
        for limit, passes in ((2 * slice_bytes + 7, 3), (slice_bytes, 6)):
            api.lda_set_workspace_limit(limit)
            capped = api.lda_acc_stats(x, ent, C.NUM_CLASSES, segments=segments)
            assert api.lda_last_timings()["passes"] == passes >= 3
            check(api, c, capped, 9, "capped", segments, limit)
            assert bits_equal(capped, acc)
        api.lda_set_workspace_limit(slice_bytes - 1)
        with pytest.raises(api.KhError, match="workspace limit of %d bytes does not hold one slice's partial sums: %d bytes needed"
                           % (slice_bytes - 1, slice_bytes)):
            api.lda_acc_stats(x, ent, C.NUM_CLASSES, segments=segments)
        assert bits_equal(api.lda_acc_stats(x[:3], dict(feo=np.zeros(4, np.int64), pdf=np.zeros(0, np.int32), weight=np.zeros(0, np.float32)), 2),
                          dict(zero=np.zeros(2), first=np.zeros((2, dim)), second=np.zeros(dim * (dim + 1) // 2)))    # no item: no workspace
    finally:
        api.lda_set_workspace_limit(0)
    assert bits_equal(api.lda_acc_stats(x, ent, C.NUM_CLASSES, segments=segments), acc)         # the next call works


def posts_case(rng, T, num_pdfs):
    """Frames of 0, 1 and 3 entries in ascending pdf order; weights multiples of 2^-10, some below 0.25, some negative."""
    posts = []
    for _ in range(T):
        k = int(rng.choice([0, 1, 1, 1, 3]))
        posts.append([(int(p), float(w)) for p, w in zip(sorted(rng.choice(num_pdfs, k, replace=False)),
                                                         rng.choice([1.0, 0.5, 0.25, 0.125, 0.0625, -0.5, -0.125], k))])
    return posts


def test_segments_grouped_into_calls(api):
    """[0, 40, 70, 70, T] in one call against the same utterances in two calls with `into`: equal bits in all three
    statistics and equal draws; a call without segments is another tree (one segment), within the bound of it."""
    rng = np.random.default_rng(42)
    T, D, nc = 150, 13, 5
    feats = (rng.standard_normal((T, D)) * 2 + 0.5).astype(np.float32)
    posts = posts_case(rng, T, nc)
    x = dev(feats)
    whole = api.accumulate_lda_stats(x, posts, nc, rand_prune=0.25, seed=1, segments=[0, 40, 70, 70, T])
    part = api.accumulate_lda_stats(x[:70], posts[:70], nc, rand_prune=0.25, seed=1, segments=[0, 40, 70])
    out = api.accumulate_lda_stats(x[70:], posts[70:], nc, rand_prune=0.25, seed=1, segments=[0, 0, T - 70], into=part)
    assert out is part and bits_equal(whole, part) and whole["draws"] == part["draws"] > 0
    one = api.accumulate_lda_stats(x, posts, nc, rand_prune=0.25, seed=1)
    assert one["draws"] == whole["draws"] and np.array_equal(one["zero"], whole["zero"])
    M.srand(1)
    ent = api.lda_entries(posts)
    ent["weight"] = np.array([M.rand_prune(v, 0.25) for v in ent["weight"]], np.float32)
    c = dict(feats=feats, ent=ent, num_classes=nc)
    xi, wi, ci = C.items_of(feats, ent)
    print("one segment worst error / bound", check(api, c, one, 6, "one segment"),
          "utterances as segments", C.check_bound(whole, xi, wi, ci, 6, "segments"))
    with pytest.raises(api.KhError, match="dimension or classes count mismatch, 5, 13,  vs. 6, 13"):
        api.accumulate_lda_stats(x, posts, nc + 1, into=part)
    a = api.accumulate_lda_stats(x, posts, nc)
    both = api.add_lda_stats(api.accumulate_lda_stats(x, posts, nc), a)
    assert all(np.array_equal(both[k], 2 * a[k]) for k in KEYS)


def test_refusals_leave_the_library_working(api):
    D = api.lda_max_dim()
    c = C.kernel_case(5, 40, 4)
    ent, nc = c["ent"], c["num_classes"]
    x = dev(c["feats"])
    T = len(c["feats"])
    with pytest.raises(api.KhError, match="feature dimension %d, supported 1 ... %d" % (D + 1, D)):
        api.lda_acc_stats(torch.zeros((T, D + 1), device="cuda"), ent, nc)
    bad = dict(ent, pdf=ent["pdf"].copy())
    bad["pdf"][2] = nc
    with pytest.raises(api.KhError, match="entry 2 names pdf %d, the accumulator has %d classes" % (nc, nc)):
        api.lda_acc_stats(x, bad, nc)
    bad["pdf"][2] = -1
    with pytest.raises(api.KhError, match="entry 2 names pdf -1, the accumulator has %d classes" % nc):
        api.lda_acc_stats(x, bad, nc)
    bad = dict(ent, feo=ent["feo"].copy())
    bad["feo"][1] = bad["feo"][-1]
    with pytest.raises(api.KhError, match="frame_entry_offsets runs backwards at frame 1"):
        api.lda_acc_stats(x, bad, nc)
    bad["feo"][0] = 1
    with pytest.raises(api.KhError, match=r"frame_entry_offsets\[0\] = 1, not 0"):
        api.lda_acc_stats(x, bad, nc)
    with pytest.raises(api.KhError, match="segment_frame_offsets runs from 0 to %d, not from 0 to %d" % (T - 1, T)):
        api.lda_acc_stats(x, ent, nc, segments=[0, T - 1])
    with pytest.raises(api.KhError, match="segment_frame_offsets runs from 1 to %d, not from 0 to %d" % (T, T)):
        api.lda_acc_stats(x, ent, nc, segments=[1, T])
    with pytest.raises(api.KhError, match="segment_frame_offsets runs backwards at segment 1"):
        api.lda_acc_stats(x, ent, nc, segments=[0, 5, 3, T])
    with pytest.raises(api.KhError, match="prune threshold -1, must be >= 0"):
        api.accumulate_lda_stats(x, [[] for _ in range(T)], nc, rand_prune=-1.0)
    acc = api.lda_acc_stats(x, ent, nc)                                  # the next call works
    print("after refusals worst error / bound", check(api, c, acc, 4, "after refusals"))


def test_no_frames_and_no_entries(api):
    none = dict(feo=np.zeros(1, np.int64), pdf=np.zeros(0, np.int32), weight=np.zeros(0, np.float32))
    x0 = torch.zeros((0, 4), device="cuda")
    out = raw_acc_stats(api, x0, none, 3, -3.25, 0)
    assert out["second"].shape == (10,) and not any(out[k].any() for k in KEYS)
    assert all((raw_acc_stats(api, x0, none, 3, -3.25, 1)[k] == -3.25).all() for k in KEYS)
    acc = api.lda_acc_stats(x0, none, 3)
    assert (acc["dim"], acc["num_classes"]) == (4, 3) and not any(acc[k].any() for k in KEYS)
    t = api.lda_last_timings()
    assert (t["items"], t["slices"], t["workgroups"], t["passes"]) == (0, 0, 0, 0)
    acc = api.accumulate_lda_stats(dev(np.ones((3, 4), np.float32)), [[], [], []], 3, segments=[0, 0, 3])
    assert acc["draws"] == 0 and not any(acc[k].any() for k in KEYS)


def test_pruning_against_the_restatement(api):
    """accumulate_lda_stats at rand_prune 0 (no draw), 0.25 and 4.0 (every survivor +-4) with seed 11 against the
    restatement's RandPrune after the same srand: the same items, `zero` bit for bit, `first` and `second` within the bound."""
    rng = np.random.default_rng(43)
    T, D, nc = 150, 13, 5
    feats = (rng.standard_normal((T, D)) * 2 + 0.5).astype(np.float32)
    posts = posts_case(rng, T, nc)
    x = dev(feats)
    ent0 = api.lda_entries(posts)
    for prune in (0.0, 0.25, 4.0):
        got = api.accumulate_lda_stats(x, posts, nc, rand_prune=prune, seed=11)
        M.srand(11)
        before = M.DRAWS[0]
        pruned = np.array([M.rand_prune(v, prune) for v in ent0["weight"]], np.float32)
        draws = M.DRAWS[0] - before
        assert (draws == 0) == (prune == 0.0) and got["draws"] == draws
        ent = dict(ent0, weight=pruned)
        c = dict(feats=feats, ent=ent, num_classes=nc)
        if prune == 4.0:
            assert set(np.abs(pruned).tolist()) == {0.0, 4.0}
        if prune == 0.0:
            assert np.array_equal(pruned, ent0["weight"])
        print("rand_prune", prune, "items", int((pruned != 0).sum()), "of", len(pruned), "draws", draws,
              "device worst error / bound", check(api, c, got, 5, "prune %g" % prune))
        ref = C.restate(feats, ent, nc)
        xi, wi, ci = C.items_of(feats, ent)
        print("restatement worst error / bound", C.check_bound(ref, xi, wi, ci, 5, "restatement"))
        assert np.array_equal(ref["zero"], got["zero"])
