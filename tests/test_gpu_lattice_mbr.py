"""GPU box: kh_compact_lattice_mbr (csrc/kh_latmbr.hip) against the line-by-line restatement (latmbr_restatement.py).  The
transcendentals are taken on the host with the same libm the restatement uses and the kernel only adds, multiplies and
compares doubles in the reference's order, so every output - words, iterations, the Bayes risk, every (word, posterior) of
the sausage, both time arrays, the confidences - is compared exactly, float32 bits included."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import latmbr_cases as Cs
import latmbr_restatement as R

pytestmark = pytest.mark.gpu

f32 = np.float32


def restated(api, clat, point, one_best=None, do_mbr=True):
    L = api.compact_lattice_mbr_prepare(clat)
    hyp = R.best_path_words(L, *point) if one_best is None else list(one_best)
    return R.mbr(L, point[0], point[1], hyp, do_mbr)


def check_batch(api, clats, points=None, one_bests=None, do_mbr=True, workspace_limit=None, what=""):
    got = api.compact_lattice_mbr(clats, points, one_bests, do_mbr, workspace_limit)
    pts = [Cs.IDENTITY] if points is None else points
    wants = []
    for i, c in enumerate(clats):
        row = [restated(api, c, pt, None if one_bests is None else one_bests[i], do_mbr) for pt in pts]
        for p, w in enumerate(row):
            R.assert_same(got[i][p], w, (what, i, p))
        wants.append(row)
    return got, wants


def test_empty_hypothesis_and_one_arc(api):
    """Q = 1: a lattice of epsilon arcs (the best path has no words), and a one-arc lattice against no words and its own."""
    one = Cs.chain([5])
    got, want = check_batch(api, [Cs.all_eps(), one], what="best path")
    assert len(got[0][0]["words"]) == 0 and got[0][0]["iterations"] == 1 and len(got[0][0]["sausage_stats"]) == 1
    assert got[1][0]["words"].tolist() == [5]
    check_batch(api, [Cs.all_eps(), one], one_bests=[[], []], do_mbr=False, what="given, MAP")
    got, _ = check_batch(api, [one], one_bests=[[]], do_mbr=True, what="given, MBR")
    assert got[0][0]["words"].tolist() == [5] and got[0][0]["iterations"] == 2


@pytest.mark.parametrize("n_words", [31, 32, 33])
def test_chunk_boundary(api, n_words):
    """|R| = 31, 32, 33, that is Q = 63, 65, 67 positions 0..Q: the boundary between two chunks of 64 lanes, where a1 takes the
    column in front of the chunk from memory and a3 and the backward chain are carried in registers.  The lattice is one of
    the generator's (38 or 40 states, mostly a chain), the hypothesis is given, with and without the MBR update."""
    clat = Cs.random_mbr_clat(7109, 38, p_next=0.97, spread=1.0)
    hyp = [1 + (i * 7) % 5 for i in range(n_words)]
    for do_mbr in (False, True):
        got, want = check_batch(api, [clat], one_bests=[hyp], do_mbr=do_mbr, what=(n_words, do_mbr))
        if not do_mbr:
            assert len(want[0][0]["sausage_stats"]) == 2 * n_words + 1
    assert want[0][0]["trace"]["longest_run3"] >= 2 and want[0][0]["trace"]["same_cell"] > 0


def test_insertion_run_across_lanes_63_and_64(api):
    """One arc from the first state to the last against a hypothesis of 40 words: its row of b_arc is a single run of 3s over
    q = 3..81, so the backward chain's carry crosses from lane 0 of the second chunk into lane 63 of the first."""
    clat = Cs.shortcut(40)
    hyp = Cs.shortcut_words(40)
    got, want = check_batch(api, [clat], one_bests=[hyp], do_mbr=False)
    assert want[0][0]["trace"]["longest_run3"] == 79


def test_cases_1_and_2_meet_in_one_cell(api):
    """An arc whose b_arc is 2 at q and 1 at q + 1 adds to beta_dash(s_a, q) twice, in the reference's order (:188 of q + 1
    first, then :196 of q): a word arc behind two words of the hypothesis that do not match it."""
    clat = Cs.two_paths()
    got, want = check_batch(api, [clat], one_bests=[[1, 3, 4, 2]], do_mbr=False)
    assert want[0][0]["trace"]["same_cell"] > 0


def test_state_with_70_incoming_arcs(api):
    check_batch(api, [Cs.fan_in(70)])
    check_batch(api, [Cs.fan_in(70)], one_bests=[[2, 2]], do_mbr=True)


def test_three_points_and_a_penalty(api):
    """n_points = 3 with distinct scales and a word insertion penalty; a lattice with several final states among them."""
    points = [api.score_point(), api.score_point(inv_acoustic_scale=7.0, word_ins_penalty=0.5),
              api.score_point(lm_scale=0.5, acoustic_scale=0.25, word_ins_penalty=-1.0)]
    clats = [Cs.random_mbr_clat(7005, 25, p_next=0.7, finals=3), Cs.random_mbr_clat(7107, 20, p_next=0.7, spread=1.0), Cs.several_finals()]
    got, want = check_batch(api, clats, points=points)
    assert len(set(tuple(np.asarray(w["bayes_risk"]).reshape(1).view(np.int32)) for w in want[1])) == 3


def test_generator_set_in_one_batch_stops_at_different_iterations(api):
    """The generator set of the CPU tests as one batch: pairs of one batch take 1, 2 and 3 iterations, so later rounds run
    over a shrinking set of pairs."""
    clats, csrs, hyps, wants = Cs.generator_set()
    got = api.compact_lattice_mbr(clats)
    for i, w in enumerate(wants):
        R.assert_same(got[i][0], w, i)
    its = sorted(set(w["iterations"] for w in wants))
    assert its[:3] == [1, 2, 3], its
    t = api.compact_lattice_mbr_last_timings()
    assert t["rounds"] == max(its) and t["acc_stats"] == sum(w["iterations"] for w in wants) and t["launches"] == t["rounds"]


def test_bounded_workspace_gives_the_same(api):
    """Five lattices of unequal size under a workspace limit that admits only some of them at a time: more launches than
    rounds, the same answers."""
    clats, csrs, hyps, wants = Cs.generator_set()
    pick = [0, 9, 3, 16, 11]
    sub = [clats[i] for i in pick]
    one = api.compact_lattice_mbr(sub)
    t1 = api.compact_lattice_mbr_last_timings()
    assert t1["launches"] == t1["rounds"]
    many = api.compact_lattice_mbr(sub, workspace_limit=2 * 40 * 72 * 8 * 2)
    t2 = api.compact_lattice_mbr_last_timings()
    assert t2["rounds"] == t1["rounds"] and t2["launches"] >= t2["rounds"] + 1
    for k, i in enumerate(pick):
        R.assert_same(one[k][0], wants[i], i)
        R.assert_same(many[k][0], wants[i], i)


def test_refusals(api):
    """Every KH_EINVAL case names what it refuses."""
    capi = importlib.import_module("old-kaldi-git_amd.capi")
    ok = api.compact_lattice_mbr_prepare(Cs.two_paths())
    pts = [Cs.IDENTITY]

    def refused(L, match, points=pts, hyps=None):
        with pytest.raises(capi.KhError, match=match):
            api.compact_lattice_mbr_raw([L], points, [[[1]] * len(points)] if hyps is None else hyps)

    assert api.compact_lattice_mbr_raw([ok], pts, [[[1, 2, 4]]])[0][0]["words"].tolist() == [1, 2, 4]
    nxt = ok["arc_nextstate"].copy()
    nxt[1] = 1
    refused(dict(ok, arc_nextstate=nxt), r"lattice 0: arc 1 \(state 1 -> 1 of 4\): input lattice must be topologically sorted")
    refused(dict(ok, start=1), "lattice 0: start state 1")
    fg = ok["final_graph"].copy()
    fg[3] = 0.5
    refused(dict(ok, final_graph=fg), r"lattice 0: state 3 of 4 \(final weight 0.5, 0")
    fg, fa = ok["final_graph"].copy(), ok["final_acoustic"].copy()
    fg[1] = fa[1] = 0.0
    refused(dict(ok, final_graph=fg, final_acoustic=fa), "lattice 0: state 1 of 4")
    for bad in (np.nan, -np.inf):
        g = ok["arc_graph"].copy()
        g[2] = bad
        refused(dict(ok, arc_graph=g), r"lattice 0: arc 2 \(state 1 -> 2\): weight")
    g = ok["arc_graph"].copy()
    g[0] = np.inf                       # Zero on the only arc into state 1
    a = ok["arc_acoustic"].copy()
    a[0] = np.inf
    refused(dict(ok, arc_graph=g, arc_acoustic=a), "lattice 0, point 0: state 1: alpha = -inf")
    with pytest.raises(capi.KhError, match="no lattices or no score points"):
        api.compact_lattice_mbr_raw([ok], [], [[]])
    lib = capi.load()
    z = np.zeros(8, np.int64)
    p = lambda x, t: x.ctypes.data_as(t)
    i32, f, d = np.zeros(8, np.int32), np.zeros(8, np.float32), np.zeros(8)
    ip, fp, lp, dp = capi.c_int32_p, capi.c_float_p, capi.c_int64_p, capi.c_double_p
    rc = lib.kh_compact_lattice_mbr(1, p(i32, ip), p(i32, ip), p(z, lp), p(i32, ip), p(i32, ip), p(f, fp), p(f, fp), p(f, fp), p(f, fp),
                                    p(i32, ip), 0, p(d, dp), p(f, fp), p(z, lp), p(i32, ip), 1, p(i32, ip), p(z, lp), p(i32, ip), p(f, fp),
                                    p(f, fp), p(d, dp), p(i32, ip), p(i32, ip), p(z, lp), p(i32, ip), p(f, fp), p(i32, ip), p(z, lp),
                                    p(i32, ip), p(f, fp))
    assert rc != 0 and "n_points = 0" in lib.kh_last_error().decode()


def test_tools_end_to_end(api, tmp_path, monkeypatch, capfd):
    """Both tools on a small written archive, in process and once as the recipes call them (only PATH changed), against what
    the restatement gives for the same lattices: the ctm byte for byte."""
    keyed = Cs.small_archive()
    monkeypatch.chdir(tmp_path)
    rs = Cs.write_lats(tmp_path / "in.lats", keyed)
    ctm_tool, mbr_tool = importlib.import_module("tools.lattice_to_ctm_conf"), importlib.import_module("tools.lattice_mbr_decode")
    pt = api.score_point(inv_acoustic_scale=9.0)
    want = Cs.restated_mbr([c for _, c in keyed], [pt])
    want_ctm = "".join("".join(ctm_tool.ctm_lines(k, row[0], 0.01)) for (k, _), row in zip(keyed, want))
    want_tra = ["%s %s" % (k, "".join("%d " % w for w in row[0]["words"])) for (k, _), row in zip(keyed, want)]
    assert ctm_tool.main(["--inv-acoustic-scale=9", rs, "a.ctm"]) == 0
    assert open("a.ctm").read() == want_ctm and len(want_ctm) > 0
    assert mbr_tool.main(["--acoustic-scale=%r" % float(pt[0][3]), rs, "ark,t:a.tra", "ark,t:a.risk", "ark,t:a.sau", "ark,t:a.times"]) == 0
    assert "Done 5 lattices." in capfd.readouterr().err
    assert open("a.tra").read().splitlines() == want_tra
    cli = importlib.import_module("old-kaldi-git_amd.kaldi_cli")
    post = dict(cli.SequentialTableReader("ark:a.sau", "posterior"))
    for (k, _), row in zip(keyed, want):
        assert [[w for w, _ in b] for b in post[k]] == [[w for w, _ in b] for b in row[0]["sausage_stats"]]
    # the sweep writes per point what the plain run writes for that point
    assert ctm_tool.main(["--inv-acoustic-scales=9,12", rs, "s_LMWT.ctm"]) == 0
    assert open("s_9.ctm").read() == want_ctm
    # the given one-best with the MAP output, one utterance without a one-best
    with open("one.txt", "w") as f:
        f.write("utt_a 1 2 3\nutt_d 1 3 4\n")
    assert ctm_tool.main(["--decode-mbr=false", rs, "ark:one.txt", "g.ctm"]) == 0
    assert "No 1-best present for utterance utt_b" in capfd.readouterr().err
    sub = [(k, c) for k, c in keyed if k in ("utt_a", "utt_d")]
    given = Cs.restated_mbr([c for _, c in sub], None, [[1, 2, 3], [1, 3, 4]], False)
    assert open("g.ctm").read() == "".join("".join(ctm_tool.ctm_lines(k, row[0], 0.01)) for (k, _), row in zip(sub, given))
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    cmd = "lattice-to-ctm-conf --inv-acoustic-scale=9 %s p.ctm && lattice-mbr-decode --acoustic-scale=%r %s ark,t:p.tra" % (rs, float(pt[0][3]), rs)
    r = subprocess.run(["sh", "-c", cmd], env=env, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open("p.ctm").read() == want_ctm and open("p.tra").read().splitlines() == want_tra
