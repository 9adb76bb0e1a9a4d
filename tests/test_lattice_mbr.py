"""No device: the restatement of MinimumBayesRisk (latmbr_restatement.py) against facts that do not depend on it - closed
forms on one- and two-path lattices and on confusion networks, invariants on the generator set - then
api.compact_lattice_mbr_prepare against hand cases, and the logic of tools/lattice_mbr_decode.py and
tools/lattice_to_ctm_conf.py with the device call replaced by the restatement."""
import importlib
import math

import numpy as np
import pytest

from conftest import pkg

import latmbr_cases as Cs
import latmbr_restatement as R

f32 = np.float32
DELTA = float(f32(1.0e-05))


@pytest.fixture(scope="module")
def api():
    return pkg("api")


def restated(api, clat, words=None, do_mbr=True, point=Cs.IDENTITY):
    L = api.compact_lattice_mbr_prepare(clat)
    hyp = R.best_path_words(L, *point) if words is None else words
    return L, R.mbr(L, point[0], point[1], hyp, do_mbr)


def levenshtein(path, ref):
    D = [[max(i, j) if 0 in (i, j) else 0 for j in range(len(ref) + 1)] for i in range(len(path) + 1)]
    for i in range(1, len(path) + 1):
        for j in range(1, len(ref) + 1):
            D[i][j] = min(D[i - 1][j - 1] + (path[i - 1] != ref[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D[-1][-1]


def aligned_cost(path, ref):
    """The cheapest alignment of a word sequence to the hypothesis with its epsilon slots (one in front of, between and
    behind the words), as (errors, insertions that found no slot): a word of the path put into a slot costs l(word, slot),
    a slot left empty costs l(0, slot), a word of the path that goes into no slot - an insertion - costs 1 + delta.  Integer
    pairs compared as errors + delta * insertions, which for delta = 1e-5 is the lexicographic order."""
    slots = R.normalize_eps(ref)
    n, m = len(path), len(slots)
    D = [[None] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                D[i][j] = (0, 0)
                continue
            c = []
            if i and j:
                c.append((D[i - 1][j - 1][0] + (path[i - 1] != slots[j - 1]), D[i - 1][j - 1][1]))
            if i:
                c.append((D[i - 1][j][0] + 1, D[i - 1][j][1] + 1))
            if j:
                c.append((D[i][j - 1][0] + (slots[j - 1] != 0), D[i][j - 1][1]))
            D[i][j] = min(c)
    return D[n][m]


def test_one_path_with_its_own_words(api):
    words = [3, 1, 4, 1, 5, 9, 2, 6]
    L, r = restated(api, Cs.chain(words), words)
    assert r["bayes_risk_double"] == 0.0 and r["iterations"] == 1 and r["words"].tolist() == words
    norm = R.normalize_eps(words)
    assert [b for b in r["sausage_stats"]] == [[(w, f32(1.0))] for w in norm]
    t = [float(x) for x in L["state_times"]]
    assert r["one_best_times"].tolist() == [[t[i], t[i + 1]] for i in range(len(words))]
    assert r["one_best_confidences"].tolist() == [1.0] * len(words)


@pytest.mark.parametrize("path,ref", [([1, 2, 3], [1, 2, 3, 4]), ([1, 2, 3, 4, 5], [1, 3, 5]), ([7, 7, 7], []), ([1, 2], [3, 4, 5, 6]),
                                      ([1, 2, 3, 4], [2, 3, 4, 1]), ([5], [5, 5, 5]), ([1, 2, 3, 4, 5, 6], [1, 6]), ([4, 4, 4, 4], [9])])
def test_one_path_against_another_hypothesis(api, path, ref):
    """do_mbr=False: L is the Levenshtein distance plus delta per insertion.  An insertion in the algorithm's sense is a word of
    the path that finds no epsilon slot of the normalized hypothesis (:120: only a2 carries delta; a word put into an
    epsilon slot is a1 with l(w, 0) = 1), so the count comes from an alignment to the slots, the distance from the plain
    Levenshtein recursion."""
    _, r = restated(api, Cs.chain(path), ref, do_mbr=False)
    dist, ins = aligned_cost(path, ref)
    assert dist == levenshtein(path, ref)
    assert abs(r["bayes_risk_double"] - (dist + DELTA * ins)) <= 1e-12
    assert r["iterations"] == 1 and r["words"].tolist() == ref


@pytest.mark.parametrize("g1,g2", [(1.0, 2.25), (2.5, 0.5)])
def test_two_paths_differing_in_one_word(api, g1, g2):
    clat = Cs.two_paths(g1, g2)
    _, r = restated(api, clat)
    c2, c3 = float(f32(g1) + f32(0.5)), float(f32(g2) + f32(0.125))           # the two arcs' costs
    z = math.exp(-c2) + math.exp(-c3)
    post = {2: math.exp(-c2) / z, 3: math.exp(-c3) / z}
    bin_ = dict(r["sausage_stats"][3])                                        # bins: eps 1 eps X eps 4 eps
    assert set(bin_) == {2, 3}
    gd = r["gamma_double"][4]
    assert abs(gd[2] - post[2]) <= 1e-12 and abs(gd[3] - post[3]) <= 1e-12
    best = max(post, key=post.get)
    assert r["words"].tolist() == [1, best, 4]
    assert abs(r["bayes_risk_double"] - (1.0 - post[best])) <= 1e-12


@pytest.mark.parametrize("seed", [41, 42, 43, 44])
def test_confusion_network(api, seed):
    """Parallel arcs between consecutive states: the result is the per-bin posterior argmax and L = sum(1 - max posterior).
    No delta enters: a bin won by epsilon lies between two bins won by words (only every other bin has an epsilon arc),
    and its words go into the epsilon slot between those two, which is a1 with l(w, 0) = 1, not an insertion."""
    clat = Cs.confusion_network(seed)
    L, r = restated(api, clat)
    n_bins = int(clat["n_states"]) - 1
    want, risk = [], 0.0
    for b in range(n_bins):
        sel = np.flatnonzero(np.asarray(clat["arc_src"]) == b)
        cost = [float(f32(clat["arc_g"][j]) + f32(clat["arc_a"][j])) for j in sel]
        z = sum(math.exp(-c) for c in cost)
        post = {int(clat["arc_label"][j]): math.exp(-c) / z for j, c in zip(sel, cost)}
        best = max(post, key=post.get)
        if best != 0:
            want.append(best)
        risk += 1.0 - post[best]
    assert r["words"].tolist() == want
    assert abs(r["bayes_risk_double"] - risk) <= 1e-9


def test_generator_set_invariants():
    """About 20 generated lattices (<= 40 states, <= 4 arcs out, some with Q > 64): every gamma row sums to 1 within 1e-9
    (the reference itself only warns at 0.1; 1e-9 is six orders above the rounding of such sums at these sizes), L never
    increases between iterations by more than 1e-9, times are ordered."""
    clats, csrs, hyps, wants = Cs.generator_set()
    assert len(wants) == 20
    for L in csrs:
        assert int(L["n_states"]) <= 41 and int(np.diff(L["arc_offsets"]).max()) <= 5        # (+1: the super-final state and its arc)
    for c in clats:
        assert int(c["n_states"]) <= 40 and int(np.bincount(c["arc_src"]).max()) <= 4
    for i, w in enumerate(wants):
        for q, row in enumerate(w["gamma_double"][1:]):
            assert abs(sum(row.values()) - 1.0) <= 1e-9, (i, q)
        Ls = w["trace"]["L"]
        assert len(Ls) == w["iterations"] and all(b - a <= 1e-9 for a, b in zip(Ls, Ls[1:])), (i, Ls)
        t = w["sausage_times"]
        assert np.all(t[:, 0] <= t[:, 1]) and np.all(t[:-1, 1] <= t[1:, 0]), i
        assert len(w["one_best_times"]) == len(w["words"]) == len(w["one_best_confidences"])
    assert sum(w["iterations"] >= 2 for w in wants) >= 3
    assert sum(w["trace"]["longest_run3"] >= 2 for w in wants) >= 3
    assert sum(2 * len(h) + 1 > 64 for h in hyps) >= 2 and max(len(w["sausage_stats"]) for w in wants) > 64


# ------------------------------------------------------------------ compact_lattice_mbr_prepare
def test_prepare_several_finals(api):
    clat = Cs.several_finals()
    L = api.compact_lattice_mbr_prepare(clat)
    assert L["n_states"] == 5 and L["n_input_arcs"] == 4
    assert L["arc_offsets"].tolist() == [0, 2, 4, 6, 7, 7]
    # the epsilon arcs come behind each state's own arcs, and carry the old final weights and strings
    assert L["arc_nextstate"].tolist() == [1, 2, 3, 4, 3, 4, 4] and L["arc_label"].tolist() == [1, 2, 3, 0, 4, 0, 0]
    assert L["arc_graph"].tolist() == [0.5, 1.0, 0.25, 0.5, 0.5, 1.0, 0.125] and L["arc_acoustic"].tolist() == [0.5, 0.25, 0.5, 0.25, 1.5, 0.0, 0.5]
    assert L["perm"].tolist() == [0, 1, 2, 4, 3, 5, 6]                     # added arcs 4, 5, 6: states 1, 2, 3 in ascending order
    assert L["final_graph"].tolist() == [np.inf] * 4 + [0.0] and L["final_acoustic"].tolist() == [np.inf] * 4 + [0.0]
    assert L["arc_frames"].tolist() == [2, 3, 4, 5, 3, 4, 1] and L["state_times"].tolist() == [0, 2, 3, 6, 7]


def test_prepare_leaves_a_single_one_final_alone(api):
    clat = Cs.two_paths()
    L = api.compact_lattice_mbr_prepare(clat)
    assert L["n_states"] == 4 and L["n_input_arcs"] == 4 and L["perm"].tolist() == [0, 1, 2, 3]
    assert L["state_times"].tolist() == [0, 3, 7, 9]
    # ... but not one with a weight, a string or an arc out of it
    weighted = dict(clat, final_g=np.array([np.inf, np.inf, np.inf, 0.5], f32))
    assert api.compact_lattice_mbr_prepare(weighted)["n_states"] == 5
    string = dict(clat, final_string=[[], [], [], [7]])
    Ls = api.compact_lattice_mbr_prepare(string)
    assert Ls["n_states"] == 5 and Ls["state_times"].tolist() == [0, 3, 7, 9, 10]


def test_prepare_renumbers_what_is_not_sorted(api):
    L = api.compact_lattice_mbr_prepare(Cs.unsorted())
    assert L["n_states"] == 4 and L["start"] == 0
    assert np.all(L["arc_nextstate"] > np.repeat(np.arange(4), np.diff(L["arc_offsets"])))
    assert L["state_of"][0] == 2 and L["state_of"][3] == 1                   # the old start first, the old final last
    assert sorted(L["arc_label"].tolist()) == [1, 2, 3, 4] and L["state_times"][3] == 6
    _, r = restated(api, Cs.unsorted())
    assert len(r["words"]) == 2


# ------------------------------------------------------------------ the tools, the device call replaced by the restatement
@pytest.fixture
def tools(api, monkeypatch, tmp_path):
    monkeypatch.setattr(api, "compact_lattice_mbr", Cs.restated_mbr)
    monkeypatch.setattr(api, "select_gpu", lambda *a, **k: None)
    monkeypatch.chdir(tmp_path)
    keyed = Cs.small_archive()
    return (importlib.import_module("tools.lattice_mbr_decode"), importlib.import_module("tools.lattice_to_ctm_conf"),
            Cs.write_lats(tmp_path / "in.lats", keyed), keyed)


def test_ctm_formatting(api):
    ctm = importlib.import_module("tools.lattice_to_ctm_conf")
    r = dict(words=np.array([7, 12], np.int32), one_best_times=np.array([[0.0, 12.5], [12.5, 100.5]], f32),
             one_best_confidences=np.array([0.995, 0.12499], f32))
    # 0.01f * 12.5f = 0.125 (just below, in float: prints 0.12 or 0.13 by the float product's value), 0.995f lies above 0.995 and prints 1.00
    want = []
    for w, (a, b), c in zip([7, 12], [(0.0, 12.5), (12.5, 100.5)], [0.995, 0.12499]):
        s, d = f32(0.01) * f32(a), f32(0.01) * (f32(b) - f32(a))
        want.append("utt 1 %.2f %.2f %d %.2f\n" % (float(s), float(d), w, float(f32(c))))
    assert ctm.ctm_lines("utt", r, 0.01) == want
    assert want[0] == "utt 1 0.00 0.12 7 1.00\n" and want[1] == "utt 1 0.12 0.88 12 0.12\n"
    # times that round at the second decimal: 0.01f * 33.5f and 0.01f * 16.5f lie just below 0.335 and 0.165 as floats and
    # print 0.33 and 0.16; the products formed in double from 0.01 would print 0.34 (0.335000000000000019) and 0.17
    assert ctm.ctm_lines("u", dict(words=[3], one_best_times=[[33.5, 50.0]], one_best_confidences=[0.5]), 0.01) == ["u 1 0.33 0.16 3 0.50\n"]
    assert "%.2f %.2f" % (0.01 * 33.5, 0.01 * 16.5) == "0.34 0.17"


def test_ctm_tool_forms_and_skip(tools, capfd):
    mbr_tool, ctm_tool, rs, keyed = tools
    assert ctm_tool.main(["--acoustic-scale=0.5", rs, "plain.ctm"]) == 0
    err = capfd.readouterr().err
    pt = pkg("api").score_point(acoustic_scale=0.5)
    res = Cs.restated_mbr([c for _, c in keyed], [pt])
    want = "".join("".join(ctm_tool.ctm_lines(k, row[0], 0.01)) for (k, _), row in zip(keyed, res))
    assert open("plain.ctm").read() == want and len(want.splitlines()) == sum(len(row[0]["words"]) for row in res)
    assert "Done 5 lattices." in err and "Overall average Bayes Risk per sentence is" in err and "For utterance utt_a, Bayes Risk" in err
    # the three-argument form: MAP with given one-bests, one of them missing
    with open("one.txt", "w") as f:
        f.write("utt_a 1 2 3\nutt_b 4 5\nutt_d 1 3 4\nutt_e 3 1 4 1 5\n")
    assert ctm_tool.main(["--decode-mbr=false", "--frame-shift=0.03", rs, "ark:one.txt", "given.ctm"]) == 0
    err = capfd.readouterr().err
    assert "No 1-best present for utterance utt_c" in err and "Done 4 lattices." in err
    given = {"utt_a": [1, 2, 3], "utt_b": [4, 5], "utt_d": [1, 3, 4], "utt_e": [3, 1, 4, 1, 5]}
    kept = [(k, c) for k, c in keyed if k in given]
    res = Cs.restated_mbr([c for _, c in kept], None, [given[k] for k, _ in kept], False)
    assert open("given.ctm").read() == "".join("".join(ctm_tool.ctm_lines(k, row[0], 0.03)) for (k, _), row in zip(kept, res))
    assert [l.split()[4] for l in open("given.ctm") if l.startswith("utt_b ")] == ["4", "5"]
    # a wspecifier is refused as output; a wrong number of arguments prints the usage
    assert ctm_tool.main([rs, "ark:-"]) == 255 and "should not be a wspecifier" in capfd.readouterr().err
    assert ctm_tool.main([rs]) == 1


def test_mbr_decode_tool_every_writer(tools, capfd):
    mbr_tool, ctm_tool, rs, keyed = tools
    cli = pkg("kaldi_cli")
    assert mbr_tool.main(["--acoustic-scale=0.5", rs, "ark,t:o.tra", "ark,t:o.risk", "ark,t:o.sau", "ark,t:o.times"]) == 0
    err = capfd.readouterr().err
    res = Cs.restated_mbr([c for _, c in keyed], [pkg("api").score_point(acoustic_scale=0.5)])
    assert open("o.tra").read().splitlines() == ["%s %s" % (k, "".join("%d " % w for w in row[0]["words"])) for (k, _), row in zip(keyed, res)]
    risks = [l.split() for l in open("o.risk").read().splitlines()]
    assert [k for k, _ in risks] == [k for k, _ in keyed]
    assert [f32(v) for _, v in risks] == pytest.approx([row[0]["bayes_risk"] for row in res], rel=1e-5)
    post = dict(cli.SequentialTableReader("ark:o.sau", "posterior"))
    for (k, _), row in zip(keyed, res):
        assert [[w for w, _ in b] for b in post[k]] == [[w for w, _ in b] for b in row[0]["sausage_stats"]]
    times = open("o.times").read().splitlines()
    assert len(times) == 5 and all(len(l.split(";")) == len(row[0]["sausage_stats"]) for l, row in zip(times, res))
    tot = f32(0.0)
    for row in res:
        tot = tot + f32(row[0]["bayes_risk"])
    n_words = sum(len(row[0]["words"]) for row in res)
    assert "Done 5 lattices." in err
    assert ("Average Bayes Risk per sentence is %s and per word, %s" % (cli._cxx_float(tot / f32(5)), cli._cxx_float(tot / f32(n_words)))) in err
    # --one-best-times, binary archives, unwanted outputs left out
    assert mbr_tool.main(["--one-best-times=true", rs, "ark:o2.tra", "", "", "ark,t:o2.times"]) == 0
    capfd.readouterr()
    res = Cs.restated_mbr([c for _, c in keyed])
    assert [len(l.split(";")) if l.split()[1:] else 0 for l in open("o2.times").read().splitlines()] == [len(row[0]["words"]) for row in res]
    assert dict((k, v.tolist()) for k, v in cli.SequentialTableReader("ark:o2.tra", "int32_vector")) == {k: row[0]["words"].tolist() for (k, _), row in zip(keyed, res)}
    assert mbr_tool.main([rs]) == 1 and mbr_tool.main([rs, "a", "b", "c", "d", "e"]) == 1


def test_sweep_output_naming(tools, capfd):
    mbr_tool, ctm_tool, rs, keyed = tools
    import os
    os.makedirs("p_0.0")
    os.makedirs("p_0.5")
    assert mbr_tool.main(["--inv-acoustic-scales=9:10", "--word-ins-penalties=0.0,0.5", rs, "ark,t:p_WIP/LMWT.tra", "ark,t:p_WIP/LMWT.risk"]) == 0
    err = capfd.readouterr().err
    api = pkg("api")
    for wip in ("0.0", "0.5"):
        for lmwt in ("9", "10"):
            res = Cs.restated_mbr([c for _, c in keyed], [api.score_point(inv_acoustic_scale=float(lmwt), word_ins_penalty=float(wip))])
            assert open("p_%s/%s.tra" % (wip, lmwt)).read().splitlines() == \
                ["%s %s" % (k, "".join("%d " % w for w in row[0]["words"])) for (k, _), row in zip(keyed, res)]
            assert "[LMWT=%s WIP=%s] Done 5 lattices." % (lmwt, wip) in err
    assert ctm_tool.main(["--inv-acoustic-scales=9,11", rs, "s_LMWT.ctm"]) == 0
    capfd.readouterr()
    for lmwt in ("9", "11"):
        res = Cs.restated_mbr([c for _, c in keyed], [api.score_point(inv_acoustic_scale=float(lmwt))])
        assert open("s_%s.ctm" % lmwt).read() == "".join("".join(ctm_tool.ctm_lines(k, row[0], 0.01)) for (k, _), row in zip(keyed, res))
    # names that do not differ per point, and the sweep next to a plain scale, are refused
    assert mbr_tool.main(["--inv-acoustic-scales=9:10", rs, "ark,t:same.tra"]) == 255 and "must differ per point" in capfd.readouterr().err
    assert ctm_tool.main(["--inv-acoustic-scales=9:10", "--acoustic-scale=0.1", rs, "x_LMWT.ctm"]) == 255
