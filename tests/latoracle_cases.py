"""Hand lattices for the oracle path (csrc/kh_latoracle.hip), shared by the CPU tests (through the restatement) and the
GPU tests (through the device call).  A case is (name, clat, reference, wildcards, want): want holds the fields of the
result that the case is about - errors, correct, sub, ins, del, path_arcs (indices into the dict's arcs), words."""
import numpy as np

from latbest_restatement import make_clat

A = lambda s, d, w, string=(1,): (s, d, w, 0.0, 0.0, list(string))
FIN = lambda *states: {s: (0.0, 0.0, []) for s in states}


def chain(words, **kw):
    return make_clat(len(words) + 1, [A(i, i + 1, w) for i, w in enumerate(words)], FIN(len(words)), **kw)


def empty_reference():
    return ("empty_reference", chain([1, 2]), [], (), dict(errors=2, correct=0, sub=0, ins=2, path_arcs=[0, 1], words=[1, 2], **{"del": 0}))


def all_epsilon_lattice():
    return ("all_epsilon", chain([0, 0, 0]), [4, 5], (), dict(errors=2, correct=0, sub=0, ins=0, path_arcs=[0, 1, 2], words=[], **{"del": 2}))


def wildcard_both_sides():
    """9 is the wildcard: it is epsilon on the arc and is dropped from the reference (R = 2)."""
    return ("wildcards", chain([1, 9, 2]), [1, 9, 9, 2], (9,),
            dict(errors=0, correct=2, sub=0, ins=0, path_arcs=[0, 1, 2], words=[1, 2], **{"del": 0}))


def start_not_zero():
    """Top-sorted with start state 1: the arc out of state 0 that would match is unreachable."""
    c = make_clat(3, [A(0, 2, 5), A(1, 2, 3)], FIN(2), start=1)
    return ("start_not_zero", c, [5], (), dict(errors=1, correct=0, sub=1, ins=0, path_arcs=[1], words=[3], **{"del": 0}))


def no_final():
    c = make_clat(3, [A(0, 1, 1), A(1, 2, 2)], {})
    return ("no_final", c, [1, 2], (), dict(errors=-1))


def tie_lower_arc_number():
    """Two parallel substitutions: the lower arc number is reported."""
    c = make_clat(2, [A(0, 1, 1), A(0, 1, 2)], FIN(1))
    return ("tie_lower_arc", c, [3], (), dict(errors=1, correct=0, sub=1, ins=0, path_arcs=[0], words=[1], **{"del": 0}))


def tie_diagonal_before_insertion():
    """0 -7-> 1 -8-> 2 against [5]: D[1] = [1, 1], so at (2, 1) the arc's diagonal (D[1][0] + 1) and its insertion
    (D[1][1] + 1) both give 2: the diagonal is taken, i.e. 8 is the substitution and 7 the insertion."""
    return ("tie_diagonal", chain([7, 8]), [5], (), dict(errors=2, correct=0, sub=1, ins=1, path_arcs=[0, 1], words=[7, 8],
                                                          moves=["ins", "sub"], **{"del": 0}))


def skip_arc_picks_the_matching_path():
    """A genuinely branching lattice: the path 0 -> 2 -> 3 says [1, 2], the path 0 -> 1 -> 3 says [4, 4]."""
    c = make_clat(4, [A(0, 1, 4), A(0, 2, 1), A(1, 3, 4), A(2, 3, 2)], FIN(3))
    return ("branching", c, [1, 2], (), dict(errors=0, correct=2, sub=0, ins=0, path_arcs=[1, 3], words=[1, 2], **{"del": 0}))


def long_deletions(n=70):
    """The best alignment deletes more than 64 reference words in a row behind the lattice's one word: row 1 is
    D[1][j] = j - 1 by a run of deletions from D[1][1] = 0 that crosses the chunk boundary (the prefix-min's carry)."""
    ref = [1] + [3] * n
    return ("long_deletions", chain([1]), ref, (), dict(errors=n, correct=1, sub=0, ins=0, path_arcs=[0], words=[1], **{"del": n}))


def long_insertions(n=70):
    """... and here the lattice says more than 64 words against a one-word reference."""
    words = [1] + [3] * n
    return ("long_insertions", chain(words), [1], (), dict(errors=n, correct=1, sub=0, ins=n, path_arcs=list(range(n + 1)), words=words,
                                                            **{"del": 0}))


def all_cases():
    return [empty_reference(), all_epsilon_lattice(), wildcard_both_sides(), start_not_zero(), no_final(), tie_lower_arc_number(),
            tie_diagonal_before_insertion(), skip_arc_picks_the_matching_path(), long_deletions(), long_insertions()]


def check_result(got, want, name):
    """got: one dict of api.compact_lattice_oracle's layout (or the restatement's mapped to it)."""
    for k, v in want.items():
        if k == "moves":
            continue
        if k in ("path_arcs", "words"):
            assert list(np.asarray(got[k]).tolist()) == list(v), (name, k, got[k], v)
        else:
            assert int(got[k]) == v, (name, k, got[k], v)
