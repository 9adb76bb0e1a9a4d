"""Hand lattices for the best-path tests, the expected answer of each worked out here.  Every case: (name, CompactLattice,
(scale, penalty), expected) with expected = None (no path) or dict(words, alignment, arcs [indices into the dict's arcs],
graph_cost, acoustic_cost).  All weights are exact in float, so the expected totals are exact too."""
import numpy as np

from latbest_restatement import make_clat

IDENT = np.array([1.0, 0.0, 0.0, 1.0])


def predecessor_tie():
    """0 -> 1 -> 3 and 0 -> 2 -> 3, every arc costs 1 (graph 0.5 + acoustic 0.5), state 3 final with weight One.  Both
    paths cost 2.  State 3 is first reached from state 1 (states in number order, :1067) with 2.0; the candidate through
    state 2 is 2.0 as well, not strictly smaller (:1075), so the predecessor stays 1: words 1 3."""
    arcs = [(0, 1, 1, 0.5, 0.5, [11]), (0, 2, 2, 0.5, 0.5, [12]), (1, 3, 3, 0.5, 0.5, [13, 14]), (2, 3, 4, 0.5, 0.5, [15])]
    c = make_clat(4, arcs, {3: (0.0, 0.0, [])})
    return "predecessor_tie", c, (IDENT, 0.0), dict(words=[1, 3], alignment=[11, 13, 14], arcs=[0, 2], graph_cost=1.0, acoustic_cost=1.0)


def parallel_arc_trap():
    """0 -> 1 costs 2^30; two parallel arcs 1 -> 2: the first costs 1 + 2^-23 (word 5), the second 1 (word 6).  In double
    2^30 + 1 + 2^-23 is a tie between two neighbours spaced 2^-22 and rounds to the even one, 2^30 + 1 - the same sum the
    second arc gives.  The relaxation (:1075) therefore keeps what the FIRST arc set, but the arc of the path is chosen by
    arc cost alone (:1113): the second, cheaper one.  Words 1 6; graph total (float) 2^30 + 1 = 1073741824 (float spacing
    at 2^30 is 128, so the + 1 is lost: 1073741824.0), final weight 0.25 / 0.5 added last."""
    first = np.float32(1.0) + np.float32(2.0 ** -23)
    arcs = [(0, 1, 1, 2.0 ** 30, 0.0, [21]), (1, 2, 5, first, 0.0, [22]), (1, 2, 6, 1.0, 0.0, [23, 24])]
    c = make_clat(3, arcs, {2: (0.25, 0.5, [25])})
    return "parallel_arc_trap", c, (IDENT, 0.0), dict(words=[1, 6], alignment=[21, 23, 24, 25], arcs=[0, 2],
                                                      graph_cost=np.float32(np.float32(2.0 ** 30) + np.float32(1.0)) + np.float32(0.25),
                                                      acoustic_cost=0.5)


def unsorted_dfs_vs_kahn():
    """Arcs in this order: 0 -> 3 (word 1), 0 -> 1 (word 2), 3 -> 2 (word 3), 1 -> 2 (word 4), each costing 1; state 2 final.
    3 -> 2 goes backwards, so the lattice is not top-sorted and is renumbered (:1046-1052).  fst::TopSort: depth-first
    from 0, arcs in order: 0, 3, 2 (finish 2, finish 3), then 1 (finish 1), finish 0; reverse finishing order 0, 1, 3, 2,
    so old 1 becomes new 1 and old 3 new 2.  Both paths cost 2; the final state is reached first from new state 1 = old 1,
    which stays on the tie: words 2 4.  (Kahn's order would number old 3 before old 1 and give words 1 3.)"""
    arcs = [(0, 3, 1, 1.0, 0.0, [31]), (0, 1, 2, 1.0, 0.0, [32]), (3, 2, 3, 1.0, 0.0, [33]), (1, 2, 4, 1.0, 0.0, [34])]
    c = make_clat(4, arcs, {2: (0.0, 0.0, [35])})
    return "unsorted_dfs_vs_kahn", c, (IDENT, 0.0), dict(words=[2, 4], alignment=[32, 34, 35], arcs=[1, 3], graph_cost=2.0, acoustic_cost=0.0)


def _penalty_lattice():
    arcs = [(0, 1, 1, 0.5, 0.0, [41]), (1, 3, 2, 0.5, 0.0, [42]), (0, 2, 3, 0.75, 0.0, [43]), (2, 3, 0, 0.75, 0.0, [])]
    return make_clat(4, arcs, {3: (0.0, 0.0, [])})


def penalty_zero():
    """Two words at 0.5 each (cost 1.0) against one word at 0.75 plus a label-0 arc at 0.75 (cost 1.5): without a penalty
    the two-word path wins."""
    return "penalty_zero", _penalty_lattice(), (IDENT, 0.0), dict(words=[1, 2], alignment=[41, 42], arcs=[0, 1], graph_cost=1.0, acoustic_cost=0.0)


def penalty_one():
    """The same lattice with a word insertion penalty of 1: the two-word path costs 1.0 + 2 = 3.0, the other 1.5 + 1 = 2.5
    (the label-0 arc takes no penalty, :1140) and wins: word 3, graph total 1.75 + 0.75 = 2.5."""
    return "penalty_one", _penalty_lattice(), (IDENT, 1.0), dict(words=[3], alignment=[43], arcs=[2, 3], graph_cost=2.5, acoustic_cost=0.0)


def inv_scale_and_off_diagonal():
    """Scale matrix [[1, 0.5], [0, 0.25]]: (g, a) = (1, 2) -> (1 + 1, 0.5) = (2, 0.5); (3, 0) -> (3, 0): the first of the two
    parallel arcs wins with 2.5 against 3; final (0, 4) -> (2, 1)."""
    arcs = [(0, 1, 7, 1.0, 2.0, [51]), (0, 1, 8, 3.0, 0.0, [52])]
    c = make_clat(2, arcs, {1: (0.0, 4.0, [53])})
    return "off_diagonal", c, (np.array([1.0, 0.5, 0.0, 0.25]), 0.0), dict(words=[7], alignment=[51, 53], arcs=[0], graph_cost=4.0, acoustic_cost=1.5)


def start_is_final():
    """One state, final with weight (0.5, 0.25) and a string: the empty path, alignment = the final string."""
    c = make_clat(1, [], {0: (0.5, 0.25, [61, 62])})
    return "start_is_final", c, (IDENT, 0.0), dict(words=[], alignment=[61, 62], arcs=[], graph_cost=0.5, acoustic_cost=0.25)


def no_final_state():
    """0 -> 1 and no final weight anywhere: the super-final state never gets a predecessor (:1091), the best path is empty
    and lattice-best-path counts a failure."""
    c = make_clat(2, [(0, 1, 1, 1.0, 1.0, [71])], {})
    return "no_final_state", c, (IDENT, 0.0), None


def all_cases():
    return [f() for f in (predecessor_tie, parallel_arc_trap, unsorted_dfs_vs_kahn, penalty_zero, penalty_one,
                          inv_scale_and_off_diagonal, start_is_final, no_final_state)]


def check_result(got, want, name):
    if want is None:
        assert got is None, name
        return
    assert got is not None, name
    assert list(got["words"]) == list(want["words"]), name
    assert list(got["alignment"]) == list(want["alignment"]), name
    assert list(got["arcs"]) == list(want["arcs"]), name
    for k in ("graph_cost", "acoustic_cost"):
        assert np.float32(got[k]).view(np.int32) == np.float32(want[k]).view(np.int32), (name, k, got[k], want[k])
