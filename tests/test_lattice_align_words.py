"""CPU: the word-alignment rule of include/kaldi_hip.h at kh_compact_lattice_align_words, checked on the line-by-line
restatement (latalign_restatement.py): every aligned arc passes WordAlignedLatticeTester's conditions
(lat/word-align-lattice.cc:746-873), the aligned lattice is equivalent to its input, the numbering is topological and the
state times consistent, hand-derived results for the small cases; then the one-thread C++ baseline
(tools/latalign_cpu_baseline.cc) against the restatement bit for bit, and the two kaldi_io readers.  No device."""
import os

import numpy as np
import pytest

from conftest import ROOT, pkg

import latalign_cases as Cs
import latalign_restatement as R
import lattice_equiv as E

F = np.float32
TM = Cs.tmodel()
GOLD = os.path.join(ROOT, "tests", "golden", "kaldi_io")


def trans_state(t):
    return (t - 1) // 2            # latalign_cases: two transition-ids per HMM-state


def arc_is_valid(label, tids, wb):
    """TestArc :746-752 = TestArcSilence || TestArcNormalWord || TestArcOnePhoneWord || TestArcEmpty."""
    phone = lambda t: int(TM["tid2phone"][t])
    final = lambda t: bool(TM["tid_is_final"][t])
    loop = lambda t: bool(TM["tid_is_self_loop"][t])
    typ = lambda p: int(wb["phone_to_type"][p])
    if label == 0 and not tids:                                           # TestArcEmpty
        return True
    if not tids:
        return False
    first = phone(tids[0])

    def one_phone():                                                      # the shared tail of :767-785 and :795-813
        if any(phone(t) != first for t in tids):
            return False
        if not wb["reorder"]:
            return final(tids[-1])
        for i, t in enumerate(tids):
            if final(t):
                return all(trans_state(u) == trans_state(t) for u in tids[i + 1:])
        return False
    if label == wb["silence_label"] and typ(first) == R.NONWORD and one_phone():   # TestArcSilence
        return True
    if label != 0 and typ(first) == R.SINGLETON and one_phone():          # TestArcOnePhoneWord
        return True
    if label == 0 or typ(first) != R.BEGIN:                               # TestArcNormalWord :816-865
        return False
    num_final, i = 0, 0
    while i < len(tids):
        if final(tids[i]):
            num_final += 1
        if phone(tids[i]) != first:
            break
        i += 1
    if num_final != 1:
        return False
    while i < len(tids) and typ(phone(tids[i])) == R.INTERNAL:
        i += 1
    if i == len(tids):
        return False
    final_phone = phone(tids[i])
    if typ(final_phone) != R.END or any(phone(t) != final_phone for t in tids[i:]):
        return False
    for j in range(i, len(tids)):
        if final(tids[j]):
            if not wb["reorder"]:
                return j + 1 == len(tids)
            return all(trans_state(u) == trans_state(tids[j]) and loop(u) for u in tids[j + 1:])
    return False


def check_result(clat, res, wb, what, equivalent=True):
    """What holds for every lattice that aligned without an error.  equivalent=False: input that is not deterministic, where
    Plus drops the worse of two alignments of one word sequence, so the transition-id strings of the input are not all in
    the result (TestEquivalent :879-892 would fail on the reference's result as well); test_plus_merges_by_hand covers it."""
    assert res["status"] == R.OK, what
    for src, dst, label, g, a, tids in res["arcs"]:
        assert src < dst < res["n_states"], (what, src, dst)              # the numbering is topological
        assert arc_is_valid(label, tids, wb), (what, label, tids)
    keys = res["state_keys"]
    assert keys[0][0] == 0 and keys == sorted(keys, key=lambda k: (k[0], k[1], -len(k[3]), k[3], k[2])), what
    for src, dst, label, g, a, tids in res["arcs"]:                       # consistent state times
        assert keys[dst][0] == keys[src][0] + len(tids), (what, src, dst)
    per_state = {}
    for src, dst, label, *_ in res["arcs"]:
        per_state.setdefault(src, []).append((dst, label))
    assert all(v == sorted(set(v)) for v in per_state.values()), what     # arcs sorted by (destination, label), unique
    if wb["silence_label"] == 0 and equivalent:
        ok, diff = E.rand_equivalent(E.WordLattice.from_compact(clat), E.WordLattice.from_compact(R.to_clat(res)), num_paths=10,
                                     delta=1e-3, seed=1)
        assert ok, (what, diff)


@pytest.mark.parametrize("name", ["linear", "boundary_inside_and_at_end", "dedupe", "plus_merges", "several_finals", "shortcut"])
@pytest.mark.parametrize("silence_label", [0, 7])
def test_cases_align_validly(name, silence_label):
    wb = Cs.wbinfo(False, silence_label, silence_label and 8)
    clat = getattr(Cs, name)()
    check_result(clat, R.align(clat, TM, wb), wb, name, equivalent=name != "plus_merges")


def test_reorder():
    wb = Cs.wbinfo(True)
    clat = Cs.linear(True)
    res = R.align(clat, TM, wb)
    check_result(clat, res, wb, "reorder")
    assert R.align(clat, TM, Cs.wbinfo(False))["status"] == R.ERROR      # the wrong --reorder is noticed (:361-365)


def test_linear_by_hand():
    """A word is cut off when the first transition-id of the next arc has been seen, so its arc carries the Times of the
    input weights up to and including that arc, and the input arc's own string; the last silence is forced out at the final
    state (its end cannot be seen) without an error and carries One."""
    clat = Cs.linear()
    res = R.align(clat, TM, Cs.wbinfo(False, 7, 8))
    s = tuple(clat["arc_string"][k].tolist() for k in range(4))
    assert res["status"] == R.OK and res["n_states"] == 5 and res["n_tuples"] == 9
    want = [(0, 1, 7, F(0.5) + F(1.0), F(1.25) + F(2.5), s[0]), (1, 2, 10, F(0.25), F(0.75), s[1]), (2, 3, 12, F(0.125), F(3.0), s[2]),
            (3, 4, 7, F(0), F(0), s[3])]
    R.assert_same(res, dict(res, arcs=want, final=np.asarray([[np.inf] * 2] * 4 + [[0, 0]], F)), "linear")


def test_forced_endings_by_hand():
    one = np.asarray([[np.inf, np.inf], [0, 0]], F)
    clat = Cs.shortcut()                                                  # no state added; a whole word forced out: no error
    res = R.align(clat, TM, Cs.wbinfo())
    R.assert_same(res, dict(status=R.OK, n_tuples=3, n_states=2, final=one,
                            arcs=[(0, 1, 10, F(1), F(1), tuple(clat["arc_string"][0].tolist()))]))
    clat = Cs.forced_partial_word()                                       # :621-624
    res = R.align(clat, TM, Cs.wbinfo(False, 7, 8))
    R.assert_same(res, dict(status=R.ERROR, n_tuples=3, n_states=2, final=one,
                            arcs=[(0, 1, 8, F(1), F(1), tuple(clat["arc_string"][0].tolist()))]))
    clat = Cs.forced_silence_not_finished()                               # :604-613
    res = R.align(clat, TM, Cs.wbinfo(False, 7, 8))
    R.assert_same(res, dict(status=R.ERROR, n_tuples=3, n_states=2, final=one,
                            arcs=[(0, 1, 7, F(1), F(1), tuple(clat["arc_string"][0].tolist()))]))
    clat = Cs.forced_words_without_ids()                                  # :574-589: the label-0 arc without a string
    res = R.align(clat, TM, Cs.wbinfo())
    R.assert_same(res, dict(status=R.ERROR, n_tuples=5, n_states=3, final=np.asarray([[np.inf] * 2] * 2 + [[0, 0]], F),
                            arcs=[(0, 1, 12, F(1.5), F(1.25), tuple(clat["arc_string"][0].tolist())), (1, 2, 0, F(0), F(0), ())]))
    assert R.align(Cs.fatal_broken_silence(), TM, Cs.wbinfo())["status"] == R.FATAL
    assert R.align(Cs.empty(), TM, Cs.wbinfo())["status"] == R.EMPTY
    with pytest.raises(R.TimesError, match="state 2 is reached after 6 and after 7"):
        R.align(Cs.inconsistent_times(), TM, Cs.wbinfo())


def test_plus_merges_by_hand():
    """The better of the two arcs 0 -> 1 and of the three arcs 2 -> 3; where the weights tie, Compare of
    CompactLatticeWeight prefers the string that is larger at the first difference."""
    clat = Cs.plus_merges()
    res = R.align(clat, TM, Cs.wbinfo())
    v2 = tuple(Cs.phone_ali(5, (0, 0, 1)))
    assert [(x[:3], float(x[3]), float(x[4])) for x in res["arcs"]] == [((0, 1, 10), 0.75, 2.5), ((1, 2, 12), 0.5, 1.25), ((2, 3, 0), 0.0, 0.0)]
    assert res["arcs"][1][5] == v2


def test_two_pending_contents_and_dedupe():
    M = R.machine(Cs.boundary_inside_and_at_end(), TM, Cs.wbinfo())
    on_1 = {(t, w) for s, t, w in M.tuples if s == 1}
    assert len(on_1) >= 2 and any(w == (10,) for _, w in on_1) and any(w == () and t for t, w in on_1)
    M = R.machine(Cs.dedupe(), TM, Cs.wbinfo())
    incoming = [dst for arcs in M.out for kind, _, _, _, dst in arcs if kind == "eps" and M.tuples[dst][0] == 3]
    assert len(incoming) == 2 and len(set(incoming)) == 1


def test_max_states_at_and_below_the_tuple_count():
    clat = Cs.boundary_inside_and_at_end()
    n = R.align(clat, TM, Cs.wbinfo())["n_tuples"]
    assert R.align(clat, TM, Cs.wbinfo(), n)["status"] == R.OK
    below = R.align(clat, TM, Cs.wbinfo(), n - 1)
    assert below["status"] == R.TOO_MANY and below["n_states"] == 0
    # :315 fires exactly where the construction holds more than max_states tuples, whatever the queue's order; the count
    # reported is max_states + 1 (the machine's own count at that moment can be larger, after an Advance over several arcs)
    for m in range(1, n):
        r = R.align(clat, TM, Cs.wbinfo(), m)
        assert (r["status"], r["n_tuples"]) == (R.TOO_MANY, m + 1), m
    assert any(len(R.machine(clat, TM, Cs.wbinfo(), m).tuples) > m + 1 for m in range(1, n))


@pytest.fixture(scope="module")
def generated():
    wb = Cs.wbinfo()
    return [(seed, lats, [R.align(c, TM, wb) for c in lats]) for seed, lats in ((s, Cs.batch(s)) for s in Cs.SEEDS)]


def test_generated_lattices(generated):
    wb = Cs.wbinfo()
    n = flagged = 0
    sizes = set()
    for seed, lats, wants in generated:
        for i, (c, w) in enumerate(zip(lats, wants)):
            n += 1
            sizes.add(int(c["n_states"]))
            assert int(c["n_states"]) <= 40 and w["state_keys"][-1][0] <= 120 if w["n_states"] else True
            if w["status"] == R.OK:
                check_result(c, w, wb, (seed, i))
            else:
                flagged += 1
    assert n == 200 and flagged * 10 <= n and len(sizes) >= 5
    assert any(any(len(x[5]) != 0 and x[0] + 1 != x[1] for x in w["arcs"]) for _, _, ws in generated for w in ws)


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.lattice_align_rate as rate
    d = str(tmp_path_factory.mktemp("latalign_cpu"))
    return rate, rate.cpu_baseline(d), d


def test_cpu_baseline_bit_for_bit(rate, generated):
    rate, exe, d = rate
    api = pkg("api")
    wb = Cs.wbinfo()
    for seed, lats, wants in generated:
        got, _ = rate.run_cpu(exe, rate.pack([api.compact_lattice_align_csr(c) for c in lats], TM, wb), d)
        for i, (g, w) in enumerate(zip(got, wants)):
            R.assert_same(g, w, (seed, i))
    names = ["linear", "boundary_inside_and_at_end", "dedupe", "plus_merges", "several_finals", "shortcut", "forced_partial_word",
             "forced_words_without_ids", "forced_silence_not_finished", "fatal_broken_silence", "empty"]
    for wb in (Cs.wbinfo(False, 7, 8), Cs.wbinfo(True, 0, 0)):
        lats = [getattr(Cs, nm)() for nm in names] + [Cs.linear(True)]
        got, _ = rate.run_cpu(exe, rate.pack([api.compact_lattice_align_csr(c) for c in lats], TM, wb), d)
        for nm, g, c in zip(names + ["linear reorder"], got, lats):
            R.assert_same(g, R.align(c, TM, wb), nm)
    clat = Cs.boundary_inside_and_at_end()
    n = R.align(clat, TM, wb)["n_tuples"]
    got, _ = rate.run_cpu(exe, rate.pack([api.compact_lattice_align_csr(clat)] * 4, TM, wb, [n, n - 1, n - 3, 2]), d)
    assert [(g["status"], g["n_tuples"]) for g in got] == [(R.align(clat, TM, wb)["status"], n), (R.TOO_MANY, n), (R.TOO_MANY, n - 2), (R.TOO_MANY, 3)]
    big = [Cs.silence_run(120), Cs.silence_run(300)]
    got, _ = rate.run_cpu(exe, rate.pack([api.compact_lattice_align_csr(c) for c in big], TM, Cs.wbinfo()), d)
    for g, c in zip(got, big):
        R.assert_same(g, R.align(c, TM, Cs.wbinfo()), "silence run")
    with pytest.raises(ValueError, match="state 2 is reached after 6 and after 7"):
        rate.run_cpu(exe, rate.pack([api.compact_lattice_align_csr(Cs.inconsistent_times())], TM, wb), d)
    data, k = rate.pack([api.compact_lattice_align_csr(clat)], TM, wb)
    with pytest.raises(ValueError, match="does not match its header"):
        rate.run_cpu(exe, (data[:-4], k), d)


def test_tid_is_final_of_the_golden_topology():
    import io
    kio = pkg("kaldi_io")
    s = kio.Stream(open(os.path.join(GOLD, "topo.bin"), "rb"))
    kio.init_kaldi_input(s)
    topo = kio.read_topology(s, True)
    triples = [(1, 0, 0), (1, 1, 1), (2, 0, 2), (2, 1, 3), (2, 2, 4), (3, 0, 2), (3, 1, 4), (3, 2, 4)]
    n_tid = sum(len(topo["entries"][topo["phone2idx"][p]][h][1]) for p, h, _ in triples)
    f = io.BytesIO()
    kio.write_transition_model(f, topo, triples, np.zeros(n_tid + 1, np.float32), True)
    tm = kio.read_transition_model(kio.Stream(io.BytesIO(f.getvalue())), True)
    assert set(tm) >= {"topo", "triples", "log_probs", "tid2pdf", "tid2phone", "tid2hmm_state", "tid_is_self_loop", "tid_is_final"}
    # phone 1 has the 3-state entry whose state 0 goes to states 0, 1 and 2 = the last: transition-ids 1, 2, 3
    assert tm["tid_is_final"][:4].tolist() == [False, False, False, True] and tm["tid_is_self_loop"][:4].tolist() == [False, True, False, False]
    want = [False]
    for p, h, _ in triples:                                               # TransitionModel::IsFinal :211-225
        entry = topo["entries"][topo["phone2idx"][p]]
        want += [dst + 1 == len(entry) for dst, _ in entry[h][1]]
    assert tm["tid_is_final"].tolist() == want and tm["tid_is_final"].dtype == bool and any(want)


def test_read_word_boundary_info(tmp_path):
    kio = pkg("kaldi_io")
    wb = kio.read_word_boundary_info(os.path.join(GOLD, "word_boundary.int"), False, 7, 8)
    assert wb["phone_to_type"].tolist() == [0, 5, 1, 4, 0, 2] and wb["phone_to_type"].dtype == np.int32
    assert (wb["reorder"], wb["silence_label"], wb["partial_word_label"]) == (False, 7, 8)
    assert kio.read_word_boundary_info(os.path.join(GOLD, "word_boundary.int"))["reorder"] is True     # WordBoundaryInfoNewOpts
    p = tmp_path / "wb"
    p.write_text("3\tsingleton \r\n1 nonword")                            # tabs, \r, no last newline
    assert kio.read_word_boundary_info(str(p))["phone_to_type"].tolist() == [0, 5, 0, 3]
    for text, msg in (("", "Empty word-boundary file"), ("1 nonword\n\n", "Invalid line"), ("1 silence\n", "Invalid line"),
                      ("x begin\n", "Invalid line"), ("1 begin end\n", "Invalid line"), ("0 begin\n", "positive")):
        p.write_text(text)
        with pytest.raises(ValueError, match=msg):
            kio.read_word_boundary_info(str(p))
    p.write_bytes(b"\0B1 begin\n")
    with pytest.raises(ValueError, match="binary"):
        kio.read_word_boundary_info(str(p))
