"""Hand lattices for the lattice-prune tests, the expected answer of each worked out here.  Every case: (name,
CompactLattice, (scale, penalty), beam, expected) with expected = dict(ok, n_states, start, kept_states, kept_arcs [indices
into the dict's states / arcs, in the output's order], arc_src, arc_dst [the output's numbering], final_kept [per surviving
state], best_final_cost)."""
import numpy as np

from latbest_restatement import make_clat

IDENT = np.array([1.0, 0.0, 0.0, 1.0])
EMPTY = dict(ok=False, n_states=0, start=-1, kept_states=[], kept_arcs=[], arc_src=[], arc_dst=[], final_kept=[])


def one_state():
    """(a) One state, start and final: forward 0, best_final_cost 0.75, nothing to prune, the state stays."""
    c = make_clat(1, [], {0: (0.5, 0.25, [7])})
    return "one_state", c, (IDENT, 0.0), 2.0, dict(ok=True, n_states=1, start=0, kept_states=[0], kept_arcs=[], arc_src=[], arc_dst=[],
                                                   final_kept=[True], best_final_cost=0.75)


def tie_at_the_cutoff():
    """(b) 0 -> 1 -> 2 costs 1 + 1, the direct arcs 0 -> 2 cost 3.0 and 3.25; beam 1.0, cutoff 3.0.  The arc at exactly 3.0
    stays, because the test is `>` (:256); the one at 3.25 goes.  No state is lost."""
    arcs = [(0, 1, 1, 0.5, 0.5, [11]), (1, 2, 2, 0.5, 0.5, [12]), (0, 2, 3, 3.0, 0.0, [13]), (0, 2, 4, 3.25, 0.0, [14])]
    c = make_clat(3, arcs, {2: (0.0, 0.0, [])})
    # CSR order of the dict's arcs: state 0: 0, 2, 3; state 1: 1
    return "tie_at_the_cutoff", c, (IDENT, 0.0), 1.0, dict(ok=True, n_states=3, start=0, kept_states=[0, 1, 2], kept_arcs=[0, 2, 1],
                                                           arc_src=[0, 0, 1], arc_dst=[1, 2, 2], final_kept=[False, False, True],
                                                           best_final_cost=2.0)


def unsorted_start_not_zero():
    """(c) Start state 2; arcs 2 -> 0, 0 -> 3, 1 -> 0, each costing 1; state 3 final.  2 -> 0 and 1 -> 0 go backwards, so the
    lattice is sorted first (:193-194).  fst::TopSort: depth-first from the start state 2: 2, 0, 3 (finish 3, 0, 2), then
    from state 1 (finish 1); reverse finishing order 1, 2, 0, 3.  The sorted start state is 1, and the state in front of it
    (old 1) is unreachable: forward cost +inf, its arc is pruned (:256: inf > cutoff) and Connect drops it.  The survivors
    are old 2, 0, 3, numbered 0, 1, 2."""
    arcs = [(2, 0, 1, 1.0, 0.0, [21]), (0, 3, 2, 1.0, 0.0, [22]), (1, 0, 3, 1.0, 0.0, [23])]
    c = make_clat(4, arcs, {3: (0.0, 0.0, [24])}, start=2)
    return "unsorted_start_not_zero", c, (IDENT, 0.0), 1.0, dict(ok=True, n_states=3, start=0, kept_states=[2, 0, 3], kept_arcs=[0, 1],
                                                                 arc_src=[0, 1], arc_dst=[1, 2], final_kept=[False, False, True],
                                                                 best_final_cost=2.0)


def sorted_start_two():
    """(c) Every arc ascends (0 -> 2, 2 -> 3, 1 -> 3) and the start state is 2: the lattice has kTopSorted and keeps its
    numbering (compact_lattice_prune_order: None); states 0 and 1 lie in front of the start state and disappear."""
    arcs = [(0, 2, 1, 1.0, 0.0, [31]), (2, 3, 2, 1.0, 0.0, [32]), (1, 3, 3, 1.0, 0.0, [33])]
    c = make_clat(4, arcs, {3: (0.0, 0.0, [])}, start=2)
    return "sorted_start_two", c, (IDENT, 0.0), 1.0, dict(ok=True, n_states=2, start=0, kept_states=[2, 3], kept_arcs=[1], arc_src=[0],
                                                          arc_dst=[1], final_kept=[False, True], best_final_cost=1.0)


def no_reachable_final():
    """(d) 0 -> 1, and the only final state, 2, cannot be reached: best_final_cost = cutoff = +inf, no comparison with it is
    true, nothing is pruned by cost - and nothing is connected: the empty lattice, PruneLattice returns false."""
    c = make_clat(3, [(0, 1, 1, 1.0, 0.0, [41])], {2: (0.0, 0.0, [])})
    return "no_reachable_final", c, (IDENT, 0.0), 1.0, dict(EMPTY, best_final_cost=np.inf)


def rounding():
    """(e) 0 -> 1 -> 2 -> 3 against the direct arc 0 -> 3, weights of widely different exponents, beam 1.0.  For the arcs
    0 -> 1 and 1 -> 2 the sum p + (a + b) of :252-253 equals the cutoff exactly, while for 2 -> 3 the forward cost
    (p + a) + a' has been rounded the other way and exceeds it by one ulp: 0 -> 1 and 1 -> 2 pass the cost test, 2 -> 3
    fails it, state 2 has no way out left and Connect removes states 1 and 2 with the two arcs.  What is left is the
    direct arc."""
    h = float.fromhex
    arcs = [(0, 1, 1, h("0x1.49a9e6p+9"), 0.0, [51]), (1, 2, 2, h("0x1.080e94p-24"), 0.0, [52]), (2, 3, 3, h("0x1.d71632p-24"), 0.0, [53]),
            (0, 3, 4, h("0x1.4929e6p+9"), h("0x1.6f926p-23"), [54])]
    c = make_clat(4, arcs, {3: (0.0, 0.0, [])})
    want = dict(ok=True, n_states=2, start=0, kept_states=[0, 3], kept_arcs=[3], arc_src=[0], arc_dst=[1], final_kept=[False, True],
                best_final_cost=np.float64(np.float32(h("0x1.4929e6p+9"))) + np.float64(np.float32(h("0x1.6f926p-23"))))
    return "rounding", c, (IDENT, 0.0), 1.0, want


def scaled_there_and_back():
    """For the plain tool with --inv-acoustic-scale=12 (not one of all_cases(): its weights change).  Acoustic values times
    float(1/12), then times the DOUBLE 1 / float(1/12): 3 -> 0.25 -> 3, but 7 -> 0.5833334 -> 7.0000005 (0x1.c00002p+2), so
    the weights written are not the input's bits.  With beam 4 the arc of graph cost 40 goes."""
    arcs = [(0, 1, 1, 1.5, 3.0, [1]), (0, 1, 2, 2.0, 7.0, [2]), (0, 1, 3, 40.0, 1.0, [3])]
    return make_clat(2, arcs, {1: (0.5, 6.0, [9])})


def all_cases():
    return [one_state(), tie_at_the_cutoff(), unsorted_start_not_zero(), sorted_start_two(), no_reachable_final(), rounding()]


def check_result(got, want, name, clat):
    """got: a dict of api.compact_lattice_prune's layout (or the restatement's); the weights carried are the input's (every
    case uses the identity point and penalty 0)."""
    assert bool(got["ok"]) == want["ok"], name
    assert int(got["n_states"]) == want["n_states"] and int(got["start"]) == want["start"], name
    for k in ("kept_states", "kept_arcs", "arc_src", "arc_dst"):
        assert list(np.asarray(got[k]).tolist()) == want[k], (name, k, got[k])
    assert [bool(x != np.float32(np.inf)) for x in got["final_g"]] == want["final_kept"], name
    ka, ks = np.asarray(want["kept_arcs"], np.int64), np.asarray(want["kept_states"], np.int64)
    assert np.array_equal(np.asarray(got["arc_label"]), np.asarray(clat["arc_label"])[ka]), name
    # g + 0.0f and 1.0 * g + 0.0 * a leave a finite weight's value as it is
    assert np.array_equal(np.asarray(got["arc_g"], np.float32), np.asarray(clat["arc_g"], np.float32)[ka]), name
    assert np.array_equal(np.asarray(got["arc_a"], np.float32), np.asarray(clat["arc_a"], np.float32)[ka]), name
    assert all(np.array_equal(x, clat["arc_string"][j]) for x, j in zip(got["arc_string"], ka)), name
    for x, s, k in zip(got["final_string"], ks, want["final_kept"]):
        assert np.array_equal(x, clat["final_string"][s] if k else np.zeros(0, np.int32)), name
