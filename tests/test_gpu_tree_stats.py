"""GPU: kh_tree_acc_stats against the line-by-line restatement (tests/tree_stats_restatement.py: numpy float32 products,
float64 adds one frame after another), BIT FOR BIT - the int64 views of the doubles are compared, no tolerance: the
reference's sums are fixed-order chains and the kernel keeps the order.  Shapes are the smallest at which the kernel can go
wrong: every D at which the column blocks change (1, 39, 63, 64, 65, 130 and the limit), runs of 0, 1, 2, tile - 1, tile,
tile + 1 and 2 tile + 1 frames interleaved with one another and with unused frames, a padded row pitch, hundreds of
single-frame events.  Fails without the feature: the entry points do not exist."""
import ctypes

import numpy as np
import pytest
import torch

import tree_stats_cases as C
import tree_stats_restatement as R
from conftest import pkg

pytestmark = pytest.mark.gpu


def dev(x, pad=0):
    """The rows on the device; with pad, as the leading columns of a wider tensor (row pitch D + pad)."""
    x = np.ascontiguousarray(x, np.float32)
    if not pad:
        return torch.from_numpy(x).cuda()
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=torch.float32).cuda()
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return wide[:, :x.shape[1]]


def call(api, feats, fe, E, count=None, stats=None, add=False, pad=0):
    D = feats.shape[1]
    count = np.full(E, 7.5) if count is None else count.copy()
    stats = np.full((E, 2, D), 7.5) if stats is None else stats.copy()
    api.tree_acc_stats(dev(feats, pad), fe, count, stats, add=add)
    return count, stats


@pytest.mark.parametrize("D", [1, 39, 63, 64, 65, 130, "max"])
def test_edge_runs_every_column_split(api, D):
    D = api.tree_max_dim() if D == "max" else D
    assert api.tree_max_dim() >= 512
    rng = np.random.default_rng(100 + D)
    runs = C.edge_runs(api.tree_tile())
    feats, fe, E = C.kernel_case(rng, D, runs, unused=11)
    want = R.add_stats(feats, fe, E)
    # add = 0 overwrites buffers that held 7.5, the event without a frame included
    got = call(api, feats, fe, E, pad=3 if D % 2 else 0)
    assert C.same_bits(got[0], want[0]) and C.same_bits(got[1], want[1])
    assert got[0].tolist() == [float(n) for n in runs] and not got[1][0].any()
    t = api.tree_last_timings()
    assert {k: t[k] for k in ("frames", "events", "work_items", "longest")} == C.plan_counts(fe, E, D)
    assert t["call_ms"] >= t["plan_ms"] > 0 and t["call_ms"] >= t["kernels_ms"] >= 0
    # add = 1 runs on: other frames, the events met in another order
    feats2, fe2, _ = C.kernel_case(rng, D, runs[::-1], unused=5)
    want2 = R.add_stats(feats2, fe2, E, *want)
    got2 = call(api, feats2, fe2, E, got[0], got[1], add=True, pad=5)
    assert C.same_bits(got2[0], want2[0]) and C.same_bits(got2[1], want2[1])
    assert C.same_bits(got2[1][3], want2[1][3]) and not C.same_bits(got2[1][3], got[1][3])


def test_single_frame_events(api):
    rng = np.random.default_rng(7)
    E = 700
    feats, fe, _ = C.kernel_case(rng, 39, [1] * E, unused=40)
    got, want = call(api, feats, fe, E), R.add_stats(feats, fe, E)
    assert C.same_bits(got[0], want[0]) and C.same_bits(got[1], want[1])
    assert api.tree_last_timings()["work_items"] == E and api.tree_last_timings()["longest"] == 1


def test_one_call_equals_two_calls_at_every_cut(api):
    rng = np.random.default_rng(8)
    feats, fe, E = C.kernel_case(rng, 5, [6, 1, 5], unused=2)
    whole, want = call(api, feats, fe, E), R.add_stats(feats, fe, E)
    assert C.same_bits(whole[1], want[1])
    for cut in range(len(fe) + 1):
        first = call(api, feats[:cut], fe[:cut], E)
        both = call(api, feats[cut:], fe[cut:], E, first[0], first[1], add=True)
        assert C.same_bits(both[0], whole[0]) and C.same_bits(both[1], whole[1]), cut


def test_order_sensitive_cases(api):
    for name, case in C.order_cases(np.random.default_rng(3)).items():
        assert C.sensitive(case) == (True, True, True), name
        feats, fe, E = case
        got, want = call(api, feats, fe, E), R.add_stats(feats, fe, E)
        assert C.same_bits(got[0], want[0]) and C.same_bits(got[1], want[1]), name


def test_no_frames_and_no_events(api):
    D = 40
    none = np.zeros((0, D), np.float32)
    count, stats = call(api, none, np.zeros(0, np.int32), 3)                       # T = 0: zeros
    assert not count.any() and not stats.any()
    t = api.tree_last_timings()
    assert (t["frames"], t["events"], t["work_items"], t["longest"], t["kernels_ms"]) == (0, 0, 0, 0, 0.0)
    held = (np.arange(3.0), np.arange(3.0 * 2 * D).reshape(3, 2, D))
    count, stats = call(api, none, np.zeros(0, np.int32), 3, *held, add=True)      # ... or what the buffers held
    assert C.same_bits(count, held[0]) and C.same_bits(stats, held[1])
    feats = C.features(np.random.default_rng(1), 9, D)
    count, stats = call(api, feats, np.full(9, -1, np.int32), 0)                   # E = 0: nothing to write
    assert count.shape == (0,) and stats.shape == (0, 2, D)
    count, stats = call(api, feats, np.full(9, -1, np.int32), 2, *[h[:2] for h in held], add=True)     # every frame unused
    assert C.same_bits(count, held[0][:2]) and C.same_bits(stats, held[1][:2])
    count, stats = call(api, none, np.zeros(0, np.int32), 0)
    assert count.shape == (0,)


def test_refusals_name_the_offender(api):
    capi = pkg("capi")
    lib = capi.load()
    x = torch.zeros((4, 8), dtype=torch.float32).cuda()
    count, stats = np.zeros(2), np.zeros((2, 2, 8))
    dp, ip = capi.c_double_p, capi.c_int32_p

    def refused(D, stride, fe, E=2):
        fe = np.asarray(fe, np.int32)
        rc = lib.kh_tree_acc_stats(ctypes.c_void_p(x.data_ptr()), len(fe), D, stride, fe.ctypes.data_as(ip), E, 0, count.ctypes.data_as(dp),
                                   stats.ctypes.data_as(dp))
        assert rc != 0
        return lib.kh_last_error().decode()

    big = api.tree_max_dim() + 1
    assert refused(big, big, [0]) == "kh_tree_acc_stats: feature dimension %d, supported 1 ... %d" % (big, big - 1)
    assert refused(0, 8, [0]) == "kh_tree_acc_stats: feature dimension 0, supported 1 ... %d" % (big - 1)
    assert refused(8, 7, [0]) == "kh_tree_acc_stats: feat_stride 7 is less than the feature dimension 8"
    assert refused(8, 8, [0, 1, 2, 0]) == "kh_tree_acc_stats: frame 2 names event 2, the call has 2 events (-1: frame not used)"
    assert refused(8, 8, [0, -2]) == "kh_tree_acc_stats: frame 1 names event -2, the call has 2 events (-1: frame not used)"
    assert refused(8, 8, [-1, 0], E=0) == "kh_tree_acc_stats: frame 1 names event 0, the call has 0 events (-1: frame not used)"
    with pytest.raises(api.KhError, match="3 frame events against 4 frames"):
        api.tree_acc_stats(x, np.zeros(3, np.int32), count, stats)
    assert not count.any() and not stats.any()                  # nothing was written


def test_running_accumulator(api):
    """api.TreeStats over two batches: the events a batch touches are compacted, their rows gathered, one call, scattered
    back; items() in std::map order."""
    rng = np.random.default_rng(9)
    D = 13
    events = [((-1, k % 3), (0, k // 3), (1, 5)) for k in range(9)] + [((-1, 0), (1, 2))]
    ts = api.TreeStats(D, 0.01)
    ref = {}
    for batch in range(2):
        T = 50
        which = rng.integers(-1, len(events), T) if batch == 0 else rng.integers(4, len(events), T)
        feats = C.features(rng, T, D)
        ts.accumulate(dev(feats), [None if k < 0 else events[k] for k in which])
        for t, k in enumerate(which):
            if k >= 0:
                ref.setdefault(events[k], R.GaussClusterable(D, 0.01)).add_stats(feats[t])
    got = list(ts.items())
    assert [e for e, _ in got] == sorted(ref) and len(ts) == len(ref)
    for e, g in got:
        assert g["count"] == float(ref[e].count) and C.same_bits(g["stats"], ref[e].stats) and g["var_floor"] == float(np.float32(0.01))
    # the same batches as a table of events (with repeats, and an entry no frame names) and per-frame indices
    rng = np.random.default_rng(9)
    ts2 = api.TreeStats(D, 0.01)
    table = events + events[:3] + [((-1, 2), (1, 99))]
    for batch in range(2):
        which = rng.integers(-1, len(events), 50) if batch == 0 else rng.integers(4, len(events), 50)
        codes = np.where((which >= 0) & (which < 3) & (np.arange(50) % 2 == 1), which + len(events), which)
        ts2.accumulate(dev(C.features(rng, 50, D)), table, codes=codes)
    got2 = list(ts2.items())
    assert [e for e, _ in got2] == [e for e, _ in got]
    assert all(a["count"] == b["count"] and C.same_bits(a["stats"], b["stats"]) for (_, a), (_, b) in zip(got, got2))
    with pytest.raises(api.KhError, match="a code outside -1 ... %d" % (len(table) - 1)):
        ts2.accumulate(dev(np.zeros((1, D), np.float32)), table, codes=[len(table)])
    with pytest.raises(api.KhError, match="features of dimension 12, the statistics have 13"):
        ts.accumulate(dev(np.zeros((1, 12), np.float32)), [None])
