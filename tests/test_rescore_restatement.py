"""CPU: the restatements of tests/rescore_restatement.py pinned - rescoring against sums written out, against the oracle's
RescoreLattice on state-level lattices (an independent anchor compiled from oracle/) and against per-arc float sums; every
status; Factor and ConvertLattice on hand lattices whose result follows from the rule - and kaldi_io.lattice_to_compact_lattice
(the product's ConvertLattice) held to the restatement."""
import numpy as np
import pytest

import latalign_cases as A
import lattice_equiv as E
import rescore_cases as C
import rescore_restatement as R
from conftest import pkg

F = np.float32
INF = F(np.inf)


def loglikes(seed, rows, cols=C.N_PDFS):
    return (np.random.default_rng(seed).standard_normal((rows, cols)) * 3 - 4).astype(F)


# ------------------------------------------------------------------------------------------------------------ rescoring

def test_hand_case_sums_written_out():
    """Two arcs and a final string over 5 frames; tid2pdf = identity minus one.  Every sum is written as the reference
    performs it: -log_like + old, frame after frame."""
    t2p = np.asarray([0, 0, 1, 2, 1], np.int32)        # transition-ids 2 and 4 share pdf 1
    ll = np.asarray([[0.5, 1.5, 2.5], [-1.0, -2.0, -3.0], [0.25, 0.75, 1.25], [8.0, 16.0, 32.0], [0.125, 0.0625, 0.03125]], F)
    c = A.clat(3, [(0, 1, 7, 0.5, 10.0, [1, 2]), (1, 2, 8, 0.25, -0.0, [4]), (0, 2, 9, 1.0, 1.0, [3, 3, 1])], {2: (2.0, 100.0, [2, 4])})
    status, arc_a, final_a = R.rescore_compact_lattice_internal(c, ll, t2p)
    assert status == R.OK
    assert arc_a[0] == F(F(-F(-2.0)) + F(F(-F(0.5)) + F(10.0)))                   # t = 0 pdf 0, t = 1 pdf 1: 9.5, then 11.5
    assert arc_a[2] == F(-F(0.75) + F(-0.0))                                      # arcs sorted by source: (0,1) (0,2) (1,2); t = 2 pdf 1
    assert arc_a[1] == F(-F(0.25) + F(-F(-3.0) + F(-F(2.5) + F(1.0))))            # pdf 2 at t = 0, 1; pdf 0 at t = 2: -1.5, 1.5, 1.25
    assert final_a[2] == F(-F(0.0625) + F(-F(16.0) + F(100.0)))                   # t = 3, 4, pdf 1 both
    assert (arc_a[0], arc_a[1], arc_a[2], final_a[2]) == (F(11.5), F(1.25), F(-0.75), F(83.9375))
    assert final_a[0] == INF and final_a[1] == INF                               # Zero finals untouched
    assert R.compact_lattice_state_times(c) == (5, [0, 2, 3])


def test_in_place_order_is_not_a_sum_of_the_scores():
    """Float addition in frame order: (-a + old) then -b differs from old - (a + b) for suitable values, and the
    restatement gives the former."""
    t2p = np.asarray([0, 0, 1], np.int32)
    ll = np.asarray([[F(2.0 ** 24), 0], [0, F(-1.0)]], F)
    c = A.clat(2, [(0, 1, 1, 0.0, F(2.0 ** 24), [1, 2])], {1: (0.0, 0.0, [])})
    _, arc_a, _ = R.rescore_compact_lattice_internal(c, ll, t2p)
    assert arc_a[0] == F(1.0)                                                     # (-2^24 + 2^24) = 0, then +1
    assert F(2.0 ** 24) + F(1.0) - F(2.0 ** 24) == F(0.0)                         # the other order loses the 1


def _lattice_csr(L):
    n = int(L["num_states"])
    src = np.asarray(L["arc_src"], np.int64)
    order = np.argsort(src, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    return dict(n_states=n, arc_offsets=off, arc_ilabel=np.asarray(L["arc_il"], np.int32)[order],
                arc_nextstate=np.asarray(L["arc_dst"], np.int32)[order], arc_graph=np.asarray(L["arc_g"], F)[order],
                arc_acoustic=np.asarray(L["arc_a"], F)[order], state_final=np.asarray(L["state_final"], F)), order


def short_string_clat(seed, n=12):
    """A random top-sorted CompactLattice whose strings have length 0 or 1 (what a state-level lattice converts to) with
    consistent times and empty final strings."""
    rng = np.random.default_rng(seed)
    t = np.concatenate([[0], np.cumsum(rng.integers(0, 2, n - 1))])
    t[-1] = t[-2] + 1
    arcs = []
    for s in range(n - 1):
        for d in range(s + 1, n):
            if t[d] - t[s] > 1 or (d > s + 1 and rng.random() < 0.5):
                continue
            for _ in range(int(rng.integers(1, 3))):
                arcs.append((s, d, int(rng.integers(0, 4)), float(F(rng.uniform(0, 3))), float(F(rng.uniform(-3, 3))),
                             C.tids(rng, int(t[d] - t[s]))))
    return A.clat(n, arcs, {n - 1: (0.5, 0.25, [])})


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_short_strings_equal_the_oracles_rescore_lattice_bit_for_bit(seed):
    from oracle import binding
    import os
    if not os.path.exists(binding.ORACLE_SO):
        binding.build(ref=False)
    kio = pkg("kaldi_io")
    c = short_string_clat(seed)
    t2p = C.tid2pdf()
    ll = loglikes(seed, R.compact_lattice_state_times(c)[0] + 2)
    status, arc_a, _ = R.rescore_compact_lattice_internal(c, ll, t2p)
    assert status == R.OK
    L = kio.compact_lattice_to_lattice(c)
    assert len(L["arc_src"]) == len(c["arc_src"])                                 # strings of length <= 1: arc for arc
    csr, order = _lattice_csr(L)
    want = binding.rescore_lattice(csr, ll, t2p)
    assert np.array_equal(order, np.arange(len(order)))
    assert arc_a.tobytes() == np.asarray(want, F).tobytes()
    assert (arc_a != np.asarray(c["arc_a"], F)).sum() == sum(len(x) for x in c["arc_string"])   # every id moved its arc


@pytest.mark.parametrize("make", [C.lengths_clat, C.long_final_clat, lambda: A.generate(11007, 6), lambda: A.generate(11019, 7)])
def test_longer_strings_equal_the_float_sum_arc_by_arc(make):
    c = make()
    t2p = C.tid2pdf()
    utt_len, times = R.compact_lattice_state_times(c)
    ll = loglikes(3, utt_len + 1)
    status, arc_a, final_a = R.rescore_compact_lattice_internal(c, ll, t2p)
    assert status == R.OK

    def chain(v, t, string):
        v = F(v)
        for k, tid in enumerate(string):
            v = F(F(-ll[t + k, t2p[int(tid)]]) + v)
        return v
    for j in range(len(c["arc_src"])):
        assert arc_a[j] == chain(c["arc_a"][j], times[int(c["arc_src"][j])], c["arc_string"][j]), j
    for s in range(int(c["n_states"])):
        if c["final_g"][s] == INF:
            assert final_a[s] == INF
        else:
            assert final_a[s] == chain(c["final_a"][s], times[s], c["final_string"][s]), s
    assert max(len(x) for x in c["arc_string"]) > 1


def test_empty_strings_keep_their_bits():
    c = C.negative_zero_clat()
    status, arc_a, final_a = R.rescore_compact_lattice_internal(c, loglikes(1, 3), C.tid2pdf())
    assert status == R.OK
    assert arc_a[0] == 0 and np.signbit(arc_a[0]) and final_a[2] == 0 and np.signbit(final_a[2])
    assert arc_a[1] != 0


def test_every_status():
    t2p = C.tid2pdf()
    ll = loglikes(2, 40)
    run = lambda c, m=ll: R.rescore(c, m, t2p)
    assert run(C.empty_clat()) == (R.EMPTY, None)
    assert run(C.inconsistent_clat()) == (R.INCONSISTENT_TIMES, None)
    with pytest.raises(R.Assertion, match=":87"):
        R.compact_lattice_state_times(C.inconsistent_clat())
    assert run(C.unreachable_clat()) == (R.INCONSISTENT_TIMES, None)
    assert R.compact_lattice_state_times(C.unreachable_clat())[1][1] == -1
    c = C.plain_clat()
    utt_len = R.compact_lattice_state_times(c)[0]
    assert utt_len == 12
    assert run(c, ll[:utt_len - 1]) == (R.FEATURES_TOO_SHORT, None)
    for rows in (utt_len, utt_len + 3):
        status, out = run(c, ll[:rows])
        assert status == R.OK and out is not None
    assert run(c, ll[:utt_len])[1]["arc_a"].tobytes() == run(c, ll[:utt_len + 3])[1]["arc_a"].tobytes()
    assert run(C.bad_tid_clat(0)) == (R.BAD_TID, None)
    assert run(C.bad_tid_clat(C.NUM_TIDS + 1)) == (R.BAD_TID, None)
    assert run(C.bad_tid_clat(C.NUM_TIDS))[0] == R.OK
    # a string that begins past utt_len (a dead end behind the final state): :1200-1204
    dead = A.clat(4, [(0, 1, 1, 0.0, 0.0, [1, 2]), (1, 2, 2, 0.0, 0.0, [3]), (2, 3, 3, 0.0, 0.0, [4])], {1: (0.0, 0.0, [])})
    assert run(dead) == (R.MISMATCH, None)
    # no final state: utt_len 0, nothing to rescore, the lattice comes back as it is (:101-104)
    nofinal = A.clat(2, [(0, 1, 1, 0.5, 0.5, [])], {})
    status, out = run(nofinal)
    assert status == R.OK and out["arc_a"].tobytes() == nofinal["arc_a"].tobytes()
    # final states that disagree: the maximum (:93-97)
    two = A.clat(3, [(0, 1, 1, 0.0, 0.0, [1, 2]), (1, 2, 2, 0.0, 0.0, [3])], {1: (0.0, 0.0, []), 2: (0.0, 0.0, [])})
    assert R.compact_lattice_state_times(two)[0] == 3
    # a cycle
    cyc = A.clat(3, [(0, 1, 1, 0.0, 0.0, [1]), (1, 2, 2, 0.0, 0.0, [2]), (2, 1, 3, 0.0, 0.0, [3])], {2: (0.0, 0.0, [])})
    assert run(cyc) == ("cyclic", None)


def test_unsorted_input_comes_back_top_sorted():
    c = C.unsorted_clat()
    status, out = R.rescore(c, loglikes(4, 9), C.tid2pdf())
    assert status == R.OK
    assert out["start"] == 0 and R.is_top_sorted(out)
    # DfsVisit from state 2: 2 -> 3 -> 1 (finished), then 2 -> 0; reverse finishing order 2, 0, 3, 1
    assert out["arc_src"].tolist() == [0, 0, 1, 2] and out["arc_dst"].tolist() == [2, 1, 3, 3]
    assert out["arc_label"].tolist() == [1, 2, 4, 3]


# --------------------------------------------------------------------------------------------------- Factor, ConvertLattice

def lat(n, arcs, finals, start=0):
    """arcs: (src, dst, ilabel, olabel, g, a); finals {state: (g, a)}."""
    fg, fa = np.full(n, np.inf, F), np.full(n, np.inf, F)
    for s, (g, a) in finals.items():
        fg[s], fa[s] = g, a
    return dict(num_states=n, start=start, arc_src=np.asarray([x[0] for x in arcs], np.int32), arc_dst=np.asarray([x[1] for x in arcs], np.int32),
                arc_il=np.asarray([x[2] for x in arcs], np.int32), arc_ol=np.asarray([x[3] for x in arcs], np.int32),
                arc_g=np.asarray([x[4] for x in arcs], F), arc_a=np.asarray([x[5] for x in arcs], F),
                state_final=np.where(fg == np.inf, F(np.inf), fg + fa).astype(F), state_final_graph=fg, state_final_acoustic=fa)


def arcs_of(c):
    return [(int(c["arc_src"][j]), int(c["arc_dst"][j]), int(c["arc_label"][j]), float(c["arc_g"][j]), float(c["arc_a"][j]),
             [int(x) for x in c["arc_string"][j]]) for j in range(len(c["arc_src"]))]


def finals_of(c):
    return {s: (float(c["final_g"][s]), float(c["final_a"][s])) for s in range(int(c["n_states"])) if c["final_g"][s] != INF}


HAND = {
    # a chain that merges: 0 -1:9-> 1 -2-> 2 -3-> 3(final); states 1 and 2 have one arc in, one out, no word out, not final
    "merge": (lat(4, [(0, 1, 1, 9, 0.5, 1.0), (1, 2, 2, 0, 0.25, 2.0), (2, 3, 3, 0, 0.125, 4.0)], {3: (1.0, 2.0)}),
              2, [(0, 1, 9, 0.875, 7.0, [1, 2, 3])], {1: (1.0, 2.0)}),
    # stopped by a word label on the chain's second arc: state 1 has kStateOlabelsOut
    "word_on_second_arc": (lat(3, [(0, 1, 1, 9, 0.5, 1.0), (1, 2, 2, 8, 0.25, 2.0)], {2: (0.0, 0.0)}),
                           3, [(0, 1, 9, 0.5, 1.0, [1]), (1, 2, 8, 0.25, 2.0, [2])], {2: (0.0, 0.0)}),
    # stopped by a final state in the middle
    "final_in_chain": (lat(3, [(0, 1, 1, 9, 0.5, 1.0), (1, 2, 2, 0, 0.25, 2.0)], {1: (3.0, 4.0), 2: (0.0, 0.0)}),
                       3, [(0, 1, 9, 0.5, 1.0, [1]), (1, 2, 0, 0.25, 2.0, [2])], {1: (3.0, 4.0), 2: (0.0, 0.0)}),
    # stopped by a second arc into state 2: both chains end there, the tail 2 -> 3 is an arc of its own
    "second_in_arc": (lat(4, [(0, 1, 1, 9, 0.5, 1.0), (0, 2, 5, 7, 1.5, 0.5), (1, 2, 2, 0, 0.25, 2.0), (2, 3, 3, 0, 0.125, 4.0)], {3: (0.0, 0.0)}),
                      3, [(0, 1, 9, 0.75, 3.0, [1, 2]), (0, 1, 7, 1.5, 0.5, [5]), (1, 2, 0, 0.125, 4.0, [3])], {2: (0.0, 0.0)}),
    # an epsilon arc inside a chain adds its weight and no label
    "epsilon_inside": (lat(4, [(0, 1, 1, 9, 0.5, 1.0), (1, 2, 0, 0, 0.25, 2.0), (2, 3, 3, 0, 0.125, 4.0)], {3: (0.0, 0.0)}),
                       2, [(0, 1, 9, 0.875, 7.0, [1, 3])], {1: (0.0, 0.0)}),
    # an unreachable state 3 with an arc into the final state: it stays (DfsVisit reaches it as a root of its own), and
    # TopSort's second root finishes after the first tree, so it is numbered first
    "unreachable": (lat(4, [(0, 1, 1, 9, 0.5, 1.0), (1, 2, 2, 0, 0.25, 2.0), (3, 2, 4, 6, 1.0, 1.0)], {2: (0.0, 0.0)}),
                    3, [(0, 2, 6, 1.0, 1.0, [4]), (1, 2, 9, 0.5, 1.0, [1])], None),
    # two arcs sharing a string (one symbol in Factor's table): each keeps its own copy
    "shared_string": (lat(3, [(0, 1, 1, 9, 0.5, 1.0), (0, 1, 1, 8, 0.75, 1.5), (1, 2, 2, 7, 0.0, 0.0)], {2: (0.0, 0.0)}),
                      3, [(0, 1, 9, 0.5, 1.0, [1]), (0, 1, 8, 0.75, 1.5, [1]), (1, 2, 7, 0.0, 0.0, [2])], {2: (0.0, 0.0)}),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_convert_lattice_hand_cases(name):
    L, n, arcs, finals = HAND[name]
    kio = pkg("kaldi_io")
    for what, c in (("restatement", R.convert_lattice(L)), ("kaldi_io", kio.lattice_to_compact_lattice(L))):
        assert int(c["n_states"]) == n, what
        if name == "unreachable":
            # states: 3 -> 0 (second DFS root, finished last), 0 -> 1, 2 -> 2 (state 1 is removed: one arc in, one out)
            assert c["start"] == 1, what
            assert arcs_of(c) == [(0, 2, 6, 1.0, 1.0, [4]), (1, 2, 9, 0.75, 3.0, [1, 2])], what
            assert finals_of(c) == {2: (0.0, 0.0)}, what
            continue
        assert c["start"] == 0, what
        assert arcs_of(c) == arcs, what
        assert finals_of(c) == finals, what
        assert all(len(x) == 0 for x in c["final_string"]), what


def test_factor_symbol_table_shares_strings():
    n, start, arcs, finals, symbols = R.factor(HAND["shared_string"][0])
    assert symbols == [[], [1], [2]] and [x[2] for x in arcs] == [1, 1, 2]


def test_factor_numbers_states_in_order_of_first_use():
    """0 -> 2 -> 1 with a branch 0 -> 1: discovery order 0, 2, 1; output states are created as the arcs are written: 0, then
    2 (first arc's destination), then 1."""
    L = lat(3, [(0, 2, 1, 5, 0.0, 0.0), (0, 1, 2, 6, 0.0, 0.0), (2, 1, 3, 7, 0.0, 0.0)], {1: (0.0, 0.0)})
    n, start, arcs, finals, _ = R.factor(L)
    assert (n, start) == (3, 0) and [(a[0], a[1]) for a in arcs] == [(0, 1), (0, 2), (1, 2)] and list(finals) == [2]


def shuffled(L, seed):
    """The same lattice under a random renumbering of its states (arcs listed by new source state, a state's arcs in order)."""
    rng = np.random.default_rng(seed)
    n = int(L["num_states"])
    p = rng.permutation(n)
    src = p[np.asarray(L["arc_src"], np.int64)]
    order = np.argsort(src, kind="stable")
    inv = np.argsort(p)
    out = {k: np.asarray(L[k])[order] for k in ("arc_il", "arc_ol", "arc_g", "arc_a")}
    out.update(num_states=n, start=int(p[int(L["start"])]), arc_src=src[order].astype(np.int32),
               arc_dst=p[np.asarray(L["arc_dst"], np.int64)][order].astype(np.int32))
    for k in ("state_final", "state_final_graph", "state_final_acoustic"):
        out[k] = np.asarray(L[k])[inv]
    return out


@pytest.mark.parametrize("seed", [11001, 11002, 11003, 11004, 11005, 11006])
def test_product_conversion_equals_the_restatement_and_round_trips(seed):
    """Expanded generator lattices (chains of every length), also under a shuffled numbering: kaldi_io's conversion is the
    restatement's bit for bit, and expanding the result again is path-equivalent to the input."""
    kio = pkg("kaldi_io")
    L0 = kio.compact_lattice_to_lattice(A.generate(seed, 5))
    for L in (L0, shuffled(L0, seed)):
        got, want = kio.lattice_to_compact_lattice(L), R.convert_lattice(L)
        R.same_clat(got, want, seed)
        assert got["start"] == 0 and R.is_top_sorted(got)
        assert int(got["n_states"]) < int(L["num_states"])
        back = kio.compact_lattice_to_lattice(got)
        if int(L["start"]) == 0:
            ok, diff = E.rand_equivalent(E.WordLattice.from_raw(L), E.WordLattice.from_raw(back), num_paths=30, delta=1e-3, seed=seed)
            assert ok, diff


def test_chains_of_length_one_change_only_the_numbering():
    """A state-level lattice in which no state can be removed (every inner state has two arcs in or out): the conversion
    keeps every arc, with its one transition-id as the string, under TopSort's numbering."""
    kio = pkg("kaldi_io")
    arcs = [(0, 2, 1, 5, 0.5, 1.0), (0, 2, 2, 6, 0.25, 2.0), (2, 1, 3, 7, 0.125, 3.0), (2, 1, 4, 0, 1.0, 4.0), (1, 3, 5, 8, 2.0, 5.0),
            (1, 3, 6, 0, 3.0, 6.0)]
    L = lat(4, arcs, {3: (0.5, 0.25)})
    for c in (R.convert_lattice(L), kio.lattice_to_compact_lattice(L)):
        new = {0: 0, 2: 1, 1: 2, 3: 3}
        assert arcs_of(c) == [(new[s], new[d], ol, float(F(g)), float(F(a)), [il]) for s, d, il, ol, g, a in
                              sorted(arcs, key=lambda x: new[x[0]])]
        assert finals_of(c) == {3: (0.5, 0.25)}


def test_empty_lattice_converts_to_an_empty_compact_lattice():
    kio = pkg("kaldi_io")
    L = lat(0, [], {}, start=-1)
    assert kio.lattice_to_compact_lattice(L)["n_states"] == 0 and R.convert_lattice(L)["n_states"] == 0
