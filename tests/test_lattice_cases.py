"""No GPU: the wide lattices of lattice_cases.py have the properties their GPU tests (test_gpu_lattice_forms.py) rely on to
reach a branch of csrc/kh_lattice.hip.  A shape that stops exercising what its test claims fails here, not silently there.

The limits (csrc/kh_lattice_plan.h): a value window of `win` slots holds a lattice of up to `win` states one word per state
and keeps win / 2 tagged slots for a larger one; KH_LATTICE_WIN=512 leaves 256; four workgroups per CU leave a 2048-slot value
window, a 1024-slot state-time window and LDS counters for 2816 states; one workgroup per CU 16384, 4096 and 27392; the level
preparation keeps the counters of up to 5120 states in LDS; a 64-state block stages 384 (192: more than two workgroups per
CU) arcs per wave; a level of more than 256 states takes a workgroup more than one pass."""
import numpy as np
import pytest

import lattice_cases as LC
from oracle import binding as B


@pytest.fixture(scope="module")
def shapes(oracle):
    out = {}
    for name, (T, W, fan, eps, slots) in LC.SHAPES.items():
        L = LC.make(name)
        out[name] = (L, LC.facts(L, slots))
    return out


def test_generator_builds_what_it_says():
    rng = np.random.default_rng(5)
    T, W, fan, eps = 3, 40, 2, 17
    L = LC.wide_lattice(rng, T, W, fan, eps)
    n = 1 + T * W
    src, dst, il = LC.arc_sources(L), L["arc_nextstate"].astype(np.int64), L["arc_ilabel"]
    assert L["n_states"] == n and len(src) == fan + (T - 1) * W * fan + T * W + T * eps
    assert np.all(dst > src) and np.all(dst < n)                                   # top-sorted
    assert np.array_equal(np.lexsort((dst, src)), np.arange(len(src)))             # sorted by (source, destination)
    frame = np.concatenate([[0], np.repeat(np.arange(1, T + 1), W)])
    assert np.all(frame[dst[il != 0]] == frame[src[il != 0]] + 1) and np.all(frame[dst[il == 0]] == frame[src[il == 0]])
    assert (il == 0).sum() == T * eps and il.min() >= 0 and il.max() <= 49
    emit_out = np.bincount(src[il != 0], minlength=n)
    assert np.all(emit_out[1:n - W] >= fan) and emit_out[0] >= fan and np.all(emit_out[n - W:] == 0)
    assert np.all(np.bincount(dst[il != 0], minlength=n)[1:] >= 1)                  # every state is reached
    assert np.all(L["arc_acoustic"][il == 0] == 0) and L["arc_graph"].min() >= 0 and L["arc_graph"].max() < 3
    assert np.all(np.isfinite(L["state_final"][n - W:])) and np.all(np.isinf(L["state_final"][:n - W]))
    assert L["arc_offsets"][0] == 0 and L["arc_offsets"][-1] == len(src) and np.all(np.diff(L["arc_offsets"]) >= 0)
    # add_arc keeps the order and everything else
    M = LC.add_arc(L, 3, n - 1, 7, 0.5, 0.25)
    ms, md = LC.arc_sources(M), M["arc_nextstate"].astype(np.int64)
    assert len(ms) == len(src) + 1 and np.array_equal(np.lexsort((md, ms)), np.arange(len(ms)))
    k = int(np.flatnonzero((ms == 3) & (md == n - 1) & (M["arc_ilabel"] == 7))[-1])
    for key in ("arc_ilabel", "arc_nextstate", "arc_graph", "arc_acoustic"):
        assert np.array_equal(np.delete(M[key], k), L[key])


def test_facts_on_a_known_lattice():
    """Two 64-state blocks: state 0 -> 1 ... 69, state 1 -> 69 (block 0: 70 outgoing, 63 incoming; block 1: 7 incoming)."""
    n = 70
    dst = np.concatenate([np.arange(1, 70), [69]])
    off = np.concatenate([[0, 69], np.full(n - 1, 70)]).astype(np.int64)
    L = dict(n_states=n, arc_offsets=off, arc_ilabel=np.ones(70, np.int32), arc_nextstate=dst.astype(np.int32),
             arc_graph=np.zeros(70, np.float32), arc_acoustic=np.zeros(70, np.float32), state_final=np.zeros(n, np.float32))
    f = LC.facts(L, 60)
    assert f["states"] == 70 and f["arcs"] == 70
    assert f["max_out_block"] == 70 and f["max_in_block"] == 63 and f["in_blocks_over_192"] == 0
    assert abs(f["far"] - 10 / 70) < 1e-12 and abs(f["near"] - 63 / 70) < 1e-12      # spans 1 ... 69 and 68
    assert f["widest_level"] == 68                                                   # level 1: states 1 ... 68
    lv = LC.levels(L)
    assert lv[0] == 0 and np.all(lv[1:69] == 1) and lv[69] == 2


@pytest.mark.parametrize("name,states,arcs", [("far256", 1601, 6443), ("far1024", 4401, 16703), ("far8192", 28001, 82002),
                                              ("dense", 5201, 38808)])
def test_sizes(shapes, name, states, arcs):
    L, f = shapes[name]
    assert (f["states"], f["arcs"]) == (states, arcs)


def test_far256(shapes):
    """Tagged eviction under KH_LATTICE_WIN=512 (256 slots), direct by default; backward staging overflow at 384."""
    L, f = shapes["far256"]
    print(f)
    assert 512 < f["states"] <= 2048 and f["states"] <= 2816 and f["states"] <= 5000
    assert f["far"] >= 0.2 and f["near"] > 0.0
    assert f["out_blocks_over_384"] >= 1


def test_far1024(shapes):
    """Behind fillers, four workgroups per CU: counters off LDS (> 2816), tagged in a 2048-slot window (1024 slots), the
    state-time window (1024 slots) overrun, blocks over the 192 staging both ways; alone: direct, counters in LDS."""
    L, f = shapes["far1024"]
    print(f)
    assert 2816 < f["states"] <= 5000 and 2048 < f["states"] <= 16384 and f["states"] <= 5120
    assert f["far"] >= 0.2
    assert f["in_blocks_over_192"] >= 1 and f["out_blocks_over_192"] >= 1
    # an arc from frame 2 into the last frame spans more than the state-time window (the planted inconsistency)
    T, W = LC.SHAPES["far1024"][:2]
    assert (1 + (T - 1) * W) - (2 * W) > 1024


def test_far8192(shapes):
    """Alone at the default sizes: counters off LDS (> 27392 states), tagged in the 16384-slot window (8192 slots)."""
    L, f = shapes["far8192"]
    print(f)
    assert f["states"] > 27392 and f["states"] > 16384
    assert f["far"] >= 0.2


def test_dense(shapes):
    """The level kernels: counters off LDS in the level preparation (> 5120 states), levels wider than a workgroup, blocks
    of more incoming entries than the sort's staging area (the insertion-sort branch), and more outgoing."""
    L, f = shapes["dense"]
    print(f)
    assert 5120 < f["states"] <= 16384
    assert f["widest_level"] > 256
    assert f["in_blocks_over_384"] >= 1 and f["out_blocks_over_384"] >= 1
    assert f["far"] >= 0.2
    assert shapes["far256"][1]["states"] <= 5120      # ... and sits beside a lattice that keeps its counters in LDS


@pytest.mark.parametrize("name", sorted(LC.SHAPES))
def test_oracle_is_well_conditioned_on_the_shape(shapes, name):
    """The oracle's own answer is usable as a reference: every frame's occupation sums to 1, no posterior underflows to 0,
    forward and backward totals agree, a state of frame t has time t."""
    L, _ = shapes[name]
    T, W = LC.SHAPES[name][:2]
    w = B.lattice_forward_backward(L)
    assert np.array_equal(w["state_times"], np.concatenate([[0], np.repeat(np.arange(1, T + 1), W)]))
    src, il = LC.arc_sources(L), L["arc_ilabel"]
    occ = np.bincount(w["state_times"][src[il != 0]], weights=w["arc_post"][il != 0].astype(np.float64), minlength=T)
    assert np.abs(occ - 1.0).max() < 1e-4, occ
    assert w["arc_post"].min() > 0.0 and np.isfinite(w["tot_like"])
    assert abs(w["tot_like"] - w["tot_forward"]) < 1e-8 * max(1.0, abs(w["tot_like"]))
