"""GPU box: kh_compact_lattice_align_words (csrc/kh_latalign.hip) against the line-by-line restatement
(latalign_restatement.py), field by field and bit by bit: every status, tuple count, state, final weight, arc, label, string
and both float costs.  The kernel only adds floats along a path and compares, so no tolerance is involved."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

import latalign_cases as Cs
import latalign_restatement as R
import latmbr_cases as McS

pytestmark = pytest.mark.gpu

TM = Cs.tmodel()


def check_batch(api, clats, wb, max_states=0, workspace_limit=None, what=""):
    csrs = [api.compact_lattice_align_csr(c) for c in clats]
    got = api.compact_lattice_align_words_raw(csrs, TM, wb, max_states, workspace_limit)
    ms = [max_states] * len(clats) if np.ndim(max_states) == 0 else list(max_states)
    wants = [R.align(c, TM, wb, m) for c, m in zip(clats, ms)]
    for i, (g, w) in enumerate(zip(got, wants)):
        R.assert_same(g, w, (what, i))
    return got, wants


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("labels", [(0, 0), (7, 8)])
def test_linear(api, reorder, labels):
    got, _ = check_batch(api, [Cs.linear(reorder)], Cs.wbinfo(reorder, *labels), what="linear")
    assert got[0]["status"] == R.OK and [x[2] for x in got[0]["arcs"]] == [labels[0], 10, 12, labels[0]]


def test_structure_cases(api):
    """Two pending contents on one input state; two paths into one tuple; the two Plus merges; several final states with
    weights and strings (the super-final path); the single final state that is used as it is."""
    names = ["boundary_inside_and_at_end", "dedupe", "plus_merges", "several_finals", "shortcut"]
    got, _ = check_batch(api, [getattr(Cs, n)() for n in names], Cs.wbinfo(), what="structure")
    assert [g["status"] for g in got] == [R.OK] * 5
    assert [x[:3] for x in got[2]["arcs"]] == [(0, 1, 10), (1, 2, 12), (2, 3, 0)] and got[2]["arcs"][1][5] == tuple(Cs.phone_ali(5, (0, 0, 1)))
    check_batch(api, [getattr(Cs, n)() for n in names], Cs.wbinfo(False, 7, 8), what="structure, labels")


def test_forced_endings_and_statuses(api):
    lats = [Cs.forced_partial_word(), Cs.forced_words_without_ids(), Cs.forced_silence_not_finished(), Cs.fatal_broken_silence(),
            Cs.empty(), Cs.linear()]
    for wb in (Cs.wbinfo(), Cs.wbinfo(False, 7, 8), Cs.wbinfo(True)):
        got, _ = check_batch(api, lats, wb, what="forced")
        assert [g["status"] for g in got][:5] == [R.ERROR, R.ERROR, R.ERROR, R.FATAL, R.EMPTY]
    assert got[3]["n_states"] == 0 and got[4]["n_tuples"] == 0


def test_max_states_at_and_below(api):
    clat = Cs.boundary_inside_and_at_end()
    n = R.align(clat, TM, Cs.wbinfo())["n_tuples"]
    got, _ = check_batch(api, [clat, clat, clat], Cs.wbinfo(), [n, n - 1, 0], what="max_states")
    assert [g["status"] for g in got] == [R.OK, R.TOO_MANY, R.OK] and got[1]["n_states"] == 0 and got[1]["n_tuples"] == n


def test_max_states_well_below(api):
    """n_tuples of a lattice over max_states is max_states + 1 whatever the order of exploration, on a branching lattice."""
    clat = Cs.boundary_inside_and_at_end()
    n = R.align(clat, TM, Cs.wbinfo())["n_tuples"]
    got, _ = check_batch(api, [clat] * 4, Cs.wbinfo(), [n - 2, n - 3, 2, 1], what="max_states below")
    assert [(g["status"], g["n_tuples"]) for g in got] == [(R.TOO_MANY, n - 1), (R.TOO_MANY, n - 2), (R.TOO_MANY, 3), (R.TOO_MANY, 2)]


def test_needs_more_room_runs_again(api):
    """Lattices built to overflow the first room of the tuple table (84 tuples for 2 states and 1 arc) and, with long pending
    strings copied per tuple, of the arena: the kernel ends them with its needs-more-room status, the host runs them again
    with more, and the outputs are the restatement's."""
    wb = Cs.wbinfo()
    lats = [Cs.silence_run(120), Cs.linear(), Cs.silence_run(300)]
    got, wants = check_batch(api, lats, wb, what="run again")
    t = api.compact_lattice_align_words_last_timings()
    assert t["run_again"] >= 2 and t["launches"] >= 2 and wants[0]["n_tuples"] == 122 and got[0]["status"] == R.OK
    # pending words pile up in front of every tuple (no transition-ids to cut them off): copies, not suffixes, fill the arena
    many = Cs.clat(42, [(i, i + 1, 10 + i % 5, 0.5, 0.25, []) for i in range(40)] + [(40, 41, 0, 1.0, 1.0, Cs.phone_ali(Cs.SIL))],
                   {41: (0.0, 0.0, [])})
    check_batch(api, [many], wb, what="arena")


def test_inconsistent_times_are_refused(api):
    capi = pkg("capi")
    with pytest.raises(capi.KhError, match="lattice 1: state 2 is reached after 6 and after 7 transition-ids"):
        api.compact_lattice_align_words_raw([api.compact_lattice_align_csr(c) for c in (Cs.linear(), Cs.inconsistent_times())], TM, Cs.wbinfo())
    bad = api.compact_lattice_align_csr(Cs.linear())
    nxt = bad["arc_nextstate"].copy()
    nxt[1] = 1
    with pytest.raises(capi.KhError, match=r"lattice 0: arc 1 \(state 1 -> 1 of 5\): the lattice must be top-sorted"):
        api.compact_lattice_align_words_raw([dict(bad, arc_nextstate=nxt)], TM, Cs.wbinfo())
    off = np.asarray(bad["arc_offsets"]).copy()
    off[2], off[3] = off[3], off[2]
    with pytest.raises(capi.KhError, match=r"lattice 0: state 2: arc_offsets 3, 2 of 4 arcs: the offsets must ascend"):
        api.compact_lattice_align_words_raw([dict(bad, arc_offsets=off)], TM, Cs.wbinfo())
    off = np.asarray(bad["arc_offsets"]).copy()
    off[2] = 1000
    with pytest.raises(capi.KhError, match=r"lattice 0: state 1: arc_offsets 1, 1000 of 4 arcs"):
        api.compact_lattice_align_words_raw([dict(bad, arc_offsets=off)], TM, Cs.wbinfo())
    strs = [s.copy() for s in bad["arc_string"]]
    strs[0][0] = 55
    with pytest.raises(capi.KhError, match="transition-id 55 of a model with 54"):
        api.compact_lattice_align_words_raw([dict(bad, arc_string=strs)], TM, Cs.wbinfo())


def test_two_call_sizing(api):
    """Short room: KH_EINVAL, the counts written and nothing else; the room the counts name: success."""
    capi = pkg("capi")
    lats = [Cs.linear(), Cs.several_finals()]
    csrs = [api.compact_lattice_align_csr(c) for c in lats]
    wants = [R.align(c, TM, Cs.wbinfo()) for c in lats]
    A = api.compact_lattice_align_words_pack(csrs, TM, Cs.wbinfo())
    rc, cnt, O = api.compact_lattice_align_words_call(A, [5, 5], [4, 4], [100, 100], fill=-77)
    assert rc != 0 and b"do not fit the room" in capi.load().kh_last_error()
    assert cnt["n_states"].tolist() == [w["n_states"] for w in wants] and cnt["n_arcs"].tolist() == [len(w["arcs"]) for w in wants]
    assert cnt["n_tuples"].tolist() == [w["n_tuples"] for w in wants] and cnt["status"].tolist() == [w["status"] for w in wants]
    assert cnt["n_string_words"].tolist() == [sum(len(x[5]) for x in w["arcs"]) for w in wants]
    for k in ("final_graph", "final_acoustic", "arc_src", "arc_nextstate", "arc_label", "arc_graph", "arc_acoustic", "arc_string_len", "strings"):
        assert np.all(O[k] == -77), k                                         # nothing else written
    rc, cnt2, O = api.compact_lattice_align_words_call(A, cnt["n_states"], cnt["n_arcs"], cnt["n_string_words"], fill=-77)
    assert rc == 0 and all(np.array_equal(cnt[k], cnt2[k]) for k in cnt)
    assert O["arc_label"].tolist() == [x[2] for w in wants for x in w["arcs"]] and not np.any(O["strings"] == -77)
    with pytest.raises(capi.KhError, match="lattice 1: 5 states, 5 arcs, .* do not fit the room of 5, 4, "):
        api.compact_lattice_align_words_raw(csrs, TM, Cs.wbinfo(), room=([5, 5], [4, 4], [100, 100]))
    exact = ([w["n_states"] for w in wants], [len(w["arcs"]) for w in wants], [sum(len(x[5]) for x in w["arcs"]) for w in wants])
    for g, w in zip(api.compact_lattice_align_words_raw(csrs, TM, Cs.wbinfo(), room=exact), wants):
        R.assert_same(g, w, "exact room")
    for g, w in zip(api.compact_lattice_align_words_raw(csrs, TM, Cs.wbinfo(), room=None), wants):
        R.assert_same(g, w, "guessed room")


@pytest.fixture(scope="module")
def generated():
    lats = [c for seed in Cs.SEEDS for c in Cs.batch(seed)]
    return lats, [R.align(c, TM, Cs.wbinfo()) for c in lats]


def test_generated_batch(api, generated):
    """200 lattices of mixed sizes in one call (largest first reorders them), then with a workspace limit that admits one
    lattice per launch: identical outputs."""
    lats, wants = generated
    assert len(lats) == 200 and sum(w["status"] != R.OK for w in wants) * 10 <= len(lats)
    csrs = [api.compact_lattice_align_csr(c) for c in lats]
    got = api.compact_lattice_align_words_raw(csrs, TM, Cs.wbinfo())
    for i, (g, w) in enumerate(zip(got, wants)):
        R.assert_same(g, w, ("batch", i))
    t = api.compact_lattice_align_words_last_timings()
    assert t["launches"] >= 1
    assert t["tuples"] == sum(w["n_tuples"] for w in wants)
    sub, sub_want = csrs[:24], wants[:24]
    one = api.compact_lattice_align_words_raw(sub, TM, Cs.wbinfo(), workspace_limit=1)
    for i, (g, w) in enumerate(zip(one, sub_want)):
        R.assert_same(g, w, ("one per launch", i))
    assert api.compact_lattice_align_words_last_timings()["launches"] >= 24


def test_public_call_and_reorder(api):
    """api.compact_lattice_align_words returns lattices that feed compact_lattice_mbr as they are."""
    lats = [Cs.generate(900 + i, reorder=True) for i in range(12)] + [Cs.empty()]
    wb = Cs.wbinfo(True, 7, 8)
    res = api.compact_lattice_align_words(lats, TM, wb)
    for i, (r, c) in enumerate(zip(res, lats)):
        w = R.align(c, TM, wb)
        assert r["status"] == w["status"] and r["n_tuples"] == w["n_tuples"]
        want = R.to_clat(w)
        assert (r["clat"] is None) == (want is None)
        if want is not None:
            for k in ("arc_src", "arc_dst", "arc_label", "arc_g", "arc_a", "final_g", "final_a"):
                assert np.asarray(r["clat"][k]).tobytes() == np.asarray(want[k]).tobytes(), (i, k)
            assert [x.tolist() for x in r["clat"]["arc_string"]] == [x.tolist() for x in want["arc_string"]]
    ok = [r["clat"] for r in res if r["clat"] is not None]
    assert len(api.compact_lattice_mbr(ok)) == len(ok)


def test_tool_end_to_end(api, tmp_path, monkeypatch):
    """lattice-prune | lattice-align-words | lattice-to-ctm-conf through the bin/ shims, only PATH changed: the CTM equals the
    one lattice_to_ctm_conf.py writes for the restatement's aligned lattices, byte for byte; log line and exit status, also
    where the errors outnumber the successes."""
    monkeypatch.chdir(tmp_path)
    keyed = [("utt_%02d" % i, Cs.generate(500 + i)) for i in range(6)]
    keyed.insert(3, ("utt_bad", Cs.forced_partial_word()))
    rs = McS.write_lats(tmp_path / "in.lats", keyed)
    mdl, wbf = Cs.write_model(tmp_path / "final.mdl"), Cs.write_word_boundary(tmp_path / "word_boundary.int")
    wb = Cs.wbinfo(False, 0, 0)
    prune = importlib.import_module("tools.lattice_prune")
    ctm_tool = importlib.import_module("tools.lattice_to_ctm_conf")
    cli = pkg("kaldi_cli")
    assert prune.main(["--beam=100", rs, "ark:pruned.lats"]) == 0
    pruned = list(cli.SequentialTableReader("ark:pruned.lats", "compact_lattice"))
    aligned = [(k, R.align(c, TM, wb)) for k, c in pruned]
    assert [a["status"] for _, a in aligned].count(R.ERROR) == 1
    McS.write_lats(tmp_path / "want.lats", [(k, R.to_clat(a)) for k, a in aligned])
    assert ctm_tool.main(["--inv-acoustic-scale=9", "ark:want.lats", "want.ctm"]) == 0
    want_ctm = open("want.ctm").read()
    assert len(want_ctm.splitlines()) >= 7
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    cmd = ("lattice-prune --beam=100 %s ark:- | lattice-align-words --reorder=false 'cat %s |' %s ark:- ark:- | "
           "lattice-to-ctm-conf --inv-acoustic-scale=9 ark:- got.ctm" % (rs, wbf, mdl))   # the word boundaries through a pipe
    r = subprocess.run(["sh", "-c", cmd], env=env, stderr=subprocess.PIPE, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-2000:]
    assert open("got.ctm").read() == want_ctm
    assert "Successfully aligned 6 lattices; 1 had errors." in err and "Outputting partial lattice for utt_bad" in err
    assert err.count("i.e. lattice is not deterministic.") == 1              # utt_bad's arc has no label; the others are deterministic
    # errors outnumber successes; the flagged lattice is not written; --test is refused by name
    tool = importlib.import_module("tools.lattice_align_words")
    McS.write_lats(tmp_path / "bad.lats", [("a", Cs.forced_partial_word()), ("b", Cs.empty()), ("c", Cs.linear())])
    assert tool.main(["--reorder=false", "--output-error-lats=false", wbf, mdl, "ark:bad.lats", "ark:bad_out.lats"]) == 1
    assert [k for k, _ in cli.SequentialTableReader("ark:bad_out.lats", "compact_lattice")] == ["c"]
    # with the error lattices written: still 1 aligned against 2 errors (the forced-out one is written, the empty one is not)
    assert tool.main(["--reorder=false", "--max-expand=0.001", wbf, mdl, "ark:bad.lats", "ark:ok_out.lats"]) == 1
    assert [k for k, _ in cli.SequentialTableReader("ark:ok_out.lats", "compact_lattice")] == ["a", "c"]
    assert tool.main(["--test=true", wbf, mdl, "ark:bad.lats", "ark:x.lats"]) == 255
    # fatal ends the program at that utterance; the one before it is written
    McS.write_lats(tmp_path / "fatal.lats", [("e", Cs.linear()), ("f", Cs.fatal_broken_silence()), ("g", Cs.linear())])
    assert tool.main(["--reorder=false", wbf, mdl, "ark:fatal.lats", "ark:x.lats"]) == 255
    assert [k for k, _ in cli.SequentialTableReader("ark:x.lats", "compact_lattice")] == ["e"]


def test_tool_max_expand(api, tmp_path, monkeypatch, capfd):
    """--max-expand: max_states = 1000 + 0.001 x 2 states = 1000; a lattice with 1102 tuples is counted as an error, warned
    about and not written."""
    monkeypatch.chdir(tmp_path)
    cli = pkg("kaldi_cli")
    tool = importlib.import_module("tools.lattice_align_words")
    mdl, wbf = Cs.write_model(tmp_path / "final.mdl"), Cs.write_word_boundary(tmp_path / "word_boundary.int")
    McS.write_lats(tmp_path / "in.lats", [("big", Cs.silence_run(1100)), ("c", Cs.linear()), ("d", Cs.shortcut())])
    assert tool.main(["--reorder=false", "--max-expand=0.001", wbf, mdl, "ark:in.lats", "ark:out.lats"]) == 0
    err = capfd.readouterr().err
    assert "Number of states in lattice exceeded max-states of 1000, original lattice had 2 states." in err
    assert "Successfully aligned 2 lattices; 1 had errors." in err
    assert [k for k, _ in cli.SequentialTableReader("ark:out.lats", "compact_lattice")] == ["c", "d"]
    assert tool.main(["--reorder=false", wbf, mdl, "ark:in.lats", "ark:all.lats"]) == 0
    big = dict(cli.SequentialTableReader("ark:all.lats", "compact_lattice"))["big"]
    assert int(big["n_states"]) == 1101 and len(big["arc_src"]) == 1100
