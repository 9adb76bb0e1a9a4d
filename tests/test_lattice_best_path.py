"""CPU: the best-path stage (lattice-scale | lattice-add-penalty | lattice-best-path).  The line-by-line restatement
(latbest_restatement.py) that checks the kernel on the GPU is itself checked here against brute force, against the compiled
alpha/beta oracle in the tropical semiring, and on hand lattices; the two host-only tools run end to end; the new entry
points exist and refuse to run without a device."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

import latbest_cases
import latbest_restatement as R


def _api():
    return pkg("api")


def _all_paths(csr):
    """Every (state sequence from 0 to a final state, arc sequence) of a small DAG."""
    off, nxt = csr["arc_offsets"], csr["arc_nextstate"]
    out = []

    def walk(s, arcs):
        if csr["final_graph"][s] != np.inf:
            out.append((s, list(arcs)))
        for j in range(off[s], off[s + 1]):
            arcs.append(j)
            walk(int(nxt[j]), arcs)
            arcs.pop()
    walk(0, [])
    return out


def _path_cost(arcs, final_state, g, a, fg, fa):
    """The search's own sum: left to right in double, the final weight last."""
    c = np.float64(0.0)
    for j in arcs:
        c = c + R.convert_to_cost(g[j], a[j])
    return c + R.convert_to_cost(fg[final_state], fa[final_state])


@pytest.mark.parametrize("seed", range(40))
def test_restatement_against_brute_force(seed):
    """Every path of a random DAG with at most 12 states enumerated: the restatement's total is the minimum, exactly
    (rounding is monotone, so the dynamic programme's left-to-right double sums reach the same minimum as the best
    path's), and its path is one of the minimisers."""
    rng = np.random.default_rng(seed)
    api = _api()
    n = int(rng.integers(2, 13))
    quantum = 0.25 if seed % 2 == 0 else 1.0 / 1024 * float(rng.integers(1, 7))
    clat = R.random_clat(rng, n, max_out=3, quantum=quantum, max_string=2, p_final=0.3)
    if seed % 2 == 1:       # weights that are not multiples of anything
        clat["arc_g"] = (clat["arc_g"] * np.float32(1.37)).astype(np.float32)
        clat["arc_a"] = (clat["arc_a"] * np.float32(0.73)).astype(np.float32)
    csr = api.compact_lattice_to_csr(clat)
    for scale, pen in [api.score_point(), api.score_point(inv_acoustic_scale=12.0, word_ins_penalty=0.5),
                       (np.array([1.0, 0.25, -0.125, 0.5]), np.float32(-0.75))]:
        r = R.compact_lattice_shortest_path(csr, scale, pen)
        g, a, fg, fa = R.apply_point(csr, scale, pen)
        paths = _all_paths(csr)
        assert paths and r is not None
        costs = [_path_cost(arcs, fs, g, a, fg, fa) for fs, arcs in paths]
        assert r["cost"] == min(costs)
        assert _path_cost(r["arcs"], r["final_state"], g, a, fg, fa) == min(costs)
        assert any(fs == r["final_state"] and arcs == list(r["arcs"]) for fs, arcs in paths)


@pytest.mark.parametrize("seed", range(10))
def test_restatement_against_viterbi_alphas(seed, oracle):
    """The compiled ComputeLatticeAlphasAndBetas (viterbi) on ConvertLattice of the same (scaled) CompactLattice: another
    summation order, the same optimum, so 1e-9 relative.  That routine takes a final weight as ONE float (value1 + value2)
    and adds an arc's two values in float, so the weights and the point here are dyadic (multiples of 1/64, scales 0.5 and
    0.25 + s/16, penalty 0.5): every float sum is then exact and only the order of the double sums differs."""
    from oracle import binding
    from tools.lattice_to_post import top_sorted_csr
    from tools.lattice_scale import scale_compact_lattice
    from tools.lattice_add_penalty import add_word_ins_pen
    kio, api = pkg("kaldi_io"), _api()
    rng = np.random.default_rng(100 + seed)
    clat = R.random_clat(rng, int(rng.integers(5, 200)), quantum=1.0 / 64)
    scale, pen = api.score_point(lm_scale=0.5, acoustic_scale=0.25 + seed / 16.0, word_ins_penalty=0.5)
    r = R.compact_lattice_shortest_path(api.compact_lattice_to_csr(clat), scale, pen)
    scaled = add_word_ins_pen(pen, scale_compact_lattice(scale.reshape(2, 2), clat))
    L = kio.compact_lattice_to_lattice(scaled)
    ab = binding.lattice_alphas_betas(top_sorted_csr(L, 1.0, 1.0), viterbi=True)
    assert abs(-ab["tot"] - r["cost"]) <= 1e-9 * max(1.0, abs(r["cost"]))


@pytest.mark.parametrize("case", latbest_cases.all_cases(), ids=lambda c: c[0])
def test_hand_lattices_through_the_restatement(case):
    name, clat, (scale, pen), want = case
    csr = _api().compact_lattice_to_csr(clat)
    latbest_cases.check_result(R.best_path_of_clat(clat, csr, scale, pen), want, name)


def test_unsorted_lattice_kahn_order_would_differ():
    """The hand lattice on which the numbering decides: with Kahn's order (tools/lattice_to_post.py) in place of
    fst::TopSort's the tie falls the other way."""
    name, clat, (scale, pen), want = latbest_cases.unsorted_dfs_vs_kahn()
    api = _api()
    assert list(api.compact_lattice_top_order(clat)) == [0, 1, 3, 2]
    kahn = R.make_clat(4, [(0, 1, 1, 1.0, 0.0, [31]), (0, 2, 2, 1.0, 0.0, [32]), (1, 3, 3, 1.0, 0.0, [33]), (2, 3, 4, 1.0, 0.0, [34])],
                       {3: (0.0, 0.0, [35])})       # the same lattice numbered in Kahn's order: old 3 -> 1, 1 -> 2, 2 -> 3
    got = R.best_path_of_clat(kahn, api.compact_lattice_to_csr(kahn), scale, pen)
    assert list(got["words"]) == [1, 3] and list(want["words"]) == [2, 4]
    assert api.compact_lattice_top_order(latbest_cases.predecessor_tie()[1]) is None
    cyc = R.make_clat(2, [(0, 1, 1, 0.0, 0.0, []), (1, 0, 1, 0.0, 0.0, [])], {1: (0.0, 0.0, [])})
    with pytest.raises(pkg("capi").KhError):
        api.compact_lattice_top_order(cyc)
    moved = R.make_clat(2, [(1, 0, 1, 0.0, 0.0, [])], {0: (0.0, 0.0, [])}, start=1)      # a start state != 0 is sorted, not ignored
    assert list(api.compact_lattice_top_order(moved)) == [1, 0]


def test_score_point_float_quotient():
    """--inv-acoustic-scale=12: the acoustic scale is the float 1.0f / 12.0f widened, not the double 1 / 12."""
    scale, pen = _api().score_point(inv_acoustic_scale=12.0, word_ins_penalty=0.5)
    assert scale[3] == float(np.float32(1.0) / np.float32(12.0)) and scale[3] != 1.0 / 12.0
    assert list(scale[:3]) == [1.0, 0.0, 0.0] and pen == np.float32(0.5)
    with pytest.raises(pkg("capi").KhError):
        _api().score_point(acoustic_scale=0.5, inv_acoustic_scale=2.0)


# ---------------------------------------------------------------- the host-only tools
LATS_TEXT = (b"utt1 \n"
             b"0\t1\t5\t1.5,3,7_8\n"
             b"0\t1\t0\t2,1,\n"
             b"1\t0.5,6,9\n"
             b"\n"
             b"utt2 \n"
             b"0\t1\t3\t0.25,-12,1\n"
             b"1\t2\t4\n"
             b"1\n"
             b"2\tInfinity,Infinity,\n"
             b"\n")


def _run(mod, argv):
    m = __import__("tools." + mod, fromlist=["main"])
    return m.main(argv)


def test_lattice_scale_text(tmp_path, capfd):
    """--inv-acoustic-scale=12: acoustic values times float(1/12) = 0.0833333358168602 in double, narrowed:
    3 -> 0.25 (0.2500000074505806 rounds to 0.25), 1 -> 0.08333334, 6 -> 0.5, -12 -> -1; graph values unchanged; the arc
    with weight One stays unprinted; state 2 of utt2 carries an infinite (Zero) final weight, which stays Zero and is
    therefore not a final state on output."""
    src, dst = tmp_path / "in.lats", tmp_path / "out.lats"
    src.write_bytes(LATS_TEXT)
    assert _run("lattice_scale", ["--inv-acoustic-scale=12", "ark:%s" % src, "ark,t:%s" % dst]) == 0
    assert dst.read_bytes() == (b"utt1 \n"
                                b"0\t1\t5\t1.5,0.25,7_8\n"
                                b"0\t1\t0\t2,0.08333334,\n"
                                b"1\t0.5,0.5,9\n"
                                b"\n"
                                b"utt2 \n"
                                b"0\t1\t3\t0.25,-1,1\n"
                                b"1\t2\t4\n"
                                b"1\n"
                                b"\n")
    assert "Done 2 lattices." in capfd.readouterr().err


def test_lattice_scale_all_options_and_round_trip(tmp_path):
    """[[lm, acoustic2lm], [lm2acoustic, acoustic]] = [[2, 0.5], [0.25, 0.5]] on (1.5, 3): (3 + 1.5, 0.375 + 1.5) =
    (4.5, 1.875); and text -> binary -> text is the identity."""
    src, mid, dst, back = (tmp_path / n for n in ("in.lats", "mid.lats", "out.lats", "back.lats"))
    src.write_bytes(LATS_TEXT)
    assert _run("lattice_scale", ["--lm-scale=2", "--acoustic2lm-scale=0.5", "--lm2acoustic-scale=0.25", "--acoustic-scale=0.5",
                                  "ark:%s" % src, "ark:%s" % mid]) == 0
    assert mid.read_bytes().startswith(b"utt1 \0B")
    assert _run("lattice_scale", ["ark:%s" % mid, "ark,t:%s" % dst]) == 0
    assert dst.read_bytes().splitlines()[1] == b"0\t1\t5\t4.5,1.875,7_8"
    assert _run("lattice_scale", ["ark:%s" % src, "ark:%s" % mid]) == 0
    assert _run("lattice_scale", ["ark:%s" % mid, "ark,t:%s" % back]) == 0
    assert back.read_bytes() == LATS_TEXT.replace(b"2\tInfinity,Infinity,\n", b"")


def test_lattice_add_penalty_text(tmp_path, capfd):
    """0.5 on the graph value of arcs with a word: 1.5 -> 2, 0.25 -> 0.75, the arc with weight One and word 4 -> 0.5,0,;
    the label-0 arc and the final weights stay."""
    src, dst = tmp_path / "in.lats", tmp_path / "out.lats"
    src.write_bytes(LATS_TEXT)
    assert _run("lattice_add_penalty", ["--word-ins-penalty=0.5", "ark,t:%s" % src, "ark,t:%s" % dst]) == 0
    assert dst.read_bytes() == (b"utt1 \n"
                                b"0\t1\t5\t2,3,7_8\n"
                                b"0\t1\t0\t2,1,\n"
                                b"1\t0.5,6,9\n"
                                b"\n"
                                b"utt2 \n"
                                b"0\t1\t3\t0.75,-12,1\n"
                                b"1\t2\t4\t0.5,0,\n"
                                b"1\n"
                                b"\n")
    assert "Done adding word insertion penalty to 2 lattices." in capfd.readouterr().err


def test_tools_exit_codes(tmp_path, capfd):
    """Usage (wrong argument count) and an empty archive: 1; a bad option: 255 (the binaries' -1); both acoustic scales
    set: the assertion of lattice-scale.cc:72 (abort, 134)."""
    empty, src = tmp_path / "empty.lats", tmp_path / "in.lats"
    empty.write_bytes(b"")
    src.write_bytes(LATS_TEXT)
    for mod in ("lattice_scale", "lattice_add_penalty"):
        assert _run(mod, ["ark:%s" % src]) == 1
        assert "Usage: " + mod.replace("_", "-") in capfd.readouterr().err
        assert _run(mod, ["ark:%s" % empty, "ark:/dev/null"]) == 1
        assert _run(mod, ["--no-such-option=1", "ark:%s" % src, "ark:/dev/null"]) == 255
    assert _run("lattice_scale", ["--acoustic-scale=0.5", "--inv-acoustic-scale=2", "ark:%s" % src, "ark:/dev/null"]) == 134
    assert _run("lattice_best_path", []) == 1
    assert "Usage: lattice-best-path" in capfd.readouterr().err
    assert _run("lattice_best_path", ["--no-such-option=1", "ark:%s" % src]) == 255


def test_the_two_tools_through_a_real_pipe(tmp_path):
    """bin/lattice-scale | bin/lattice-add-penalty with bin/ first in PATH, binary in between, as local/score.sh chains them."""
    src, dst = tmp_path / "in.lats", tmp_path / "out.lats"
    src.write_bytes(LATS_TEXT)
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    cmd = "lattice-scale --inv-acoustic-scale=12 ark:%s ark:- | lattice-add-penalty --word-ins-penalty=0.5 ark:- ark,t:%s" % (src, dst)
    assert subprocess.run(["sh", "-c", cmd], env=env, stderr=subprocess.DEVNULL, timeout=120).returncode == 0
    assert dst.read_bytes().splitlines()[1:3] == [b"0\t1\t5\t2,0.25,7_8", b"0\t1\t0\t2,0.08333334,"]


def test_sweep_lists_and_substitution():
    bp = pkg("kaldi_tool")
    assert bp.parse_sweep_list("9:20", "x") == [str(v) for v in range(9, 21)]
    assert bp.parse_sweep_list("0.0,0.5,1.0", "x") == ["0.0", "0.5", "1.0"]
    assert bp.substitute("ark,t:scoring/penalty_WIP/LMWT.tra", "12", "0.5") == "ark,t:scoring/penalty_0.5/12.tra"
    for bad in ("20:9", "a:b", "1,x"):
        with pytest.raises(ValueError):
            bp.parse_sweep_list(bad, "x")


def test_read_compact_lattice_keeps_the_start_state(tmp_path):
    kio = pkg("kaldi_io")
    c = kio.read_compact_lattice(io.BytesIO(b"2\t0\t5\t1,1,3\n0\n\n"), binary=False)
    assert c["start"] == 2
    buf = io.BytesIO()
    kio.write_compact_lattice(buf, latbest_cases.predecessor_tie()[1], binary=True)
    assert kio.read_compact_lattice(io.BytesIO(buf.getvalue()), binary=True)["start"] == 0
    # a start state != 0 survives the tools: lattice-scale text -> binary -> text (FstPrinter puts the start state's lines first)
    src, mid, dst = tmp_path / "in.lats", tmp_path / "mid.lats", tmp_path / "out.lats"
    src.write_bytes(b"u \n2\t0\t5\t1,1,3\n0\t1\t6\t2,2,4\n1\n\n")
    assert _run("lattice_scale", ["ark:%s" % src, "ark:%s" % mid]) == 0
    assert _run("lattice_add_penalty", ["ark:%s" % mid, "ark,t:%s" % dst]) == 0
    assert dst.read_bytes() == src.read_bytes()
    # no start state (an empty lattice): the empty best path (:1055), for every point, without a search
    empty = kio.read_compact_lattice(io.BytesIO(b"\n"), binary=False)
    assert empty["start"] == -1 and _api().compact_lattice_top_order(empty) is None
    assert _api().compact_lattice_best_paths([empty], [_api().score_point()] * 2) == [[None, None]]


# ---------------------------------------------------------------- the entry points
def test_entry_points_declared_and_loud_without_a_device():
    import torch
    capi = pkg("capi")
    lib = capi.load()
    names = ("kh_compact_lattice_best_paths", "kh_compact_lattice_best_paths_set_workspace_limit",
             "kh_compact_lattice_best_paths_last_timings")
    header = open(os.path.join(ROOT, "include", "kaldi_hip.h")).read()
    for n in names:
        assert n in capi.SIGNATURES and hasattr(lib, n) and n + "(" in header
    if torch.cuda.is_available():
        return
    api = _api()
    csr = api.compact_lattice_to_csr(latbest_cases.predecessor_tie()[1])
    with pytest.raises(capi.KhError, match="no HIP device"):
        api.compact_lattice_best_paths_raw([csr], [api.score_point()])
