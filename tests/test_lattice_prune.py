"""CPU: the pruning stage (lattice-scale | lattice-add-penalty | lattice-prune).  The line-by-line restatement
(latprune_restatement.py) that checks the kernel on the GPU is itself checked here against brute force, against the compiled
alpha/beta oracle in the tropical semiring, and on hand lattices; the tool's logic that needs no device runs; the new entry
points exist and refuse to run without a device."""
import os

import numpy as np
import pytest

from conftest import ROOT, pkg

import latprune_cases
import latprune_restatement as R


def _api():
    return pkg("api")


IDENT = np.array([1.0, 0.0, 0.0, 1.0])


@pytest.mark.parametrize("seed", range(40))
def test_restatement_against_brute_force(seed):
    """Random DAGs of at most 12 states, identity point, weights and beam multiples of 0.25: every sum is exact, so the
    surviving arcs and states are exactly the union of the start-to-final paths whose cost is <= best + beam, found by
    enumerating every path."""
    rng = np.random.default_rng(9000 + seed)
    api = _api()
    clat = R.random_clat(rng, int(rng.integers(2, 13)), max_out=3, quantum=0.25, max_string=2, p_final=0.3)
    csr = api.compact_lattice_to_prune_csr(clat)
    assert csr["start"] == 0 and api.compact_lattice_prune_order(clat) is None
    beam = 0.25 * int(rng.integers(1, 20))
    r = R.prune_lattice(csr, IDENT, 0.0, beam)
    off, nxt = csr["arc_offsets"], csr["arc_nextstate"]
    cost = lambda g, a: float(g) + float(a)
    paths = []

    def walk(s, arcs, c):
        if csr["final_graph"][s] != np.inf:
            paths.append((list(arcs), s, c + cost(csr["final_graph"][s], csr["final_acoustic"][s])))
        for j in range(off[s], off[s + 1]):
            arcs.append(j)
            walk(int(nxt[j]), arcs, c + cost(csr["arc_graph"][j], csr["arc_acoustic"][j]))
            arcs.pop()
    walk(0, [], 0.0)
    best = min(p[2] for p in paths)
    assert r["best_final_cost"] == best
    arcs, states, finals = set(), set(), set()
    src = np.repeat(np.arange(csr["n_states"]), np.diff(off))
    for path, fs, c in paths:
        if c <= best + beam:
            arcs.update(path)
            states.update([0, fs] + [int(nxt[j]) for j in path])
            finals.add(fs)
    assert set(np.flatnonzero(r["arc_keep"]).tolist()) == arcs
    assert set(np.flatnonzero(r["state_keep"]).tolist()) == states
    assert set(np.flatnonzero(r["final_keep"] & r["state_keep"]).tolist()) == finals
    assert all(r["state_keep"][src[j]] and r["state_keep"][nxt[j]] for j in arcs)


@pytest.mark.parametrize("seed", range(10))
def test_restatement_costs_against_viterbi_alphas_betas(seed, oracle):
    """The restatement's forward and backward costs against the Viterbi alphas / betas of the compiled
    ComputeLatticeAlphasAndBetas, up to sign.  That routine adds an arc's two values in float and takes a final weight as
    ONE float, so the weights are dyadic (multiples of 1/64, scales 0.5 and 0.25 + s/16, penalty 0.5) and every float sum
    is exact; 1e-9 relative is the tolerance the oracle's other users grant it.  The two share no code."""
    from oracle import binding
    api = _api()
    rng = np.random.default_rng(300 + seed)
    clat = R.random_clat(rng, int(rng.integers(5, 200)), quantum=1.0 / 64)
    scale, pen = api.score_point(lm_scale=0.5, acoustic_scale=0.25 + seed / 16.0, word_ins_penalty=0.5)
    csr = api.compact_lattice_to_prune_csr(clat)
    g, a, fg, fa = R.apply_point(csr, scale, pen)
    # forward costs alone: a beam so wide that nothing is pruned; the backward costs do not depend on the beam
    r = R.prune_lattice(csr, scale, pen, 1.0e6)
    with np.errstate(invalid="ignore"):
        fin = np.where(fg == np.inf, np.float32(np.inf), fg + fa).astype(np.float32)
    ab = binding.lattice_alphas_betas(dict(n_states=csr["n_states"], arc_offsets=csr["arc_offsets"], arc_ilabel=csr["arc_label"],
                                           arc_nextstate=csr["arc_nextstate"], arc_graph=g, arc_acoustic=a, state_final=fin),
                                      viterbi=True)
    for mine, theirs in ((r["forward"], -ab["alpha"]), (r["backward"], -ab["beta"])):
        fin_ = np.isfinite(mine)
        assert np.array_equal(fin_, np.isfinite(theirs)) and fin_.any()
        assert np.all(np.abs(mine[fin_] - theirs[fin_]) <= 1e-9 * np.maximum(1.0, np.abs(mine[fin_])))
    assert abs(r["best_final_cost"] + ab["beta"][0]) <= 1e-9 * max(1.0, abs(r["best_final_cost"]))


@pytest.mark.parametrize("case", latprune_cases.all_cases(), ids=lambda c: c[0])
def test_hand_lattices_through_the_restatement(case):
    name, clat, (scale, pen), beam, want = case
    csr = _api().compact_lattice_to_prune_csr(clat)
    latprune_cases.check_result(R.prune_clat(clat, csr, scale, pen, beam), want, name, clat)
    assert R.prune_lattice(csr, scale, pen, beam)["best_final_cost"] == want["best_final_cost"]


def test_prune_order():
    """kTopSorted does not ask where the start state is; compact_lattice_top_order (for the best-path search) does."""
    api = _api()
    c = latprune_cases.sorted_start_two()[1]
    assert api.compact_lattice_prune_order(c) is None and api.compact_lattice_top_order(c) is not None
    assert api.compact_lattice_to_prune_csr(c)["start"] == 2
    u = latprune_cases.unsorted_start_not_zero()[1]
    assert list(api.compact_lattice_prune_order(u)) == [2, 0, 1, 3]
    assert list(api.compact_lattice_prune_order(u)) == list(api.compact_lattice_top_order(u))
    csr = api.compact_lattice_to_prune_csr(u)
    assert csr["start"] == 1 and list(csr["state_of"]) == [1, 2, 0, 3] and list(csr["perm"]) == [2, 0, 1]
    cyc = R.make_clat(2, [(0, 1, 1, 0.0, 0.0, []), (1, 0, 1, 0.0, 0.0, [])], {1: (0.0, 0.0, [])})
    with pytest.raises(pkg("capi").KhError):
        api.compact_lattice_prune_order(cyc)


def test_no_final_nothing_pruned_by_cost():
    """(d): the cost test removes nothing when the cutoff is +inf; the emptiness comes from Connect."""
    name, clat, (scale, pen), beam, want = latprune_cases.no_reachable_final()
    r = R.prune_lattice(_api().compact_lattice_to_prune_csr(clat), scale, pen, beam)
    assert r["cutoff"] == np.inf and r["cost_keep"].all() and not r["state_keep"].any() and not r["arc_keep"].any()
    assert r["final_keep"][2]       # the unreachable final state keeps its weight (inf + 0 > inf is false) and is not accessible


def test_rounding_case_is_a_rounding_case():
    """(e): the arcs 0 -> 1 and 1 -> 2 pass the cost test and are dropped by reachability alone."""
    name, clat, (scale, pen), beam, want = latprune_cases.rounding()
    csr = _api().compact_lattice_to_prune_csr(clat)
    r = R.prune_lattice(csr, scale, pen, beam)
    by_dict = {int(csr["perm"][j]): j for j in range(4)}
    a01, a12, a23, a03 = (by_dict[k] for k in range(4))
    assert r["cost_keep"][a01] and r["cost_keep"][a12] and not r["cost_keep"][a23] and r["cost_keep"][a03]
    assert not r["arc_keep"][a01] and not r["arc_keep"][a12] and r["arc_keep"][a03]
    assert list(r["state_keep"]) == [True, False, False, True]
    # p + (a + b) sits on the cutoff, (p + a) + b one ulp above it
    g, a, _, _ = r["weights"]
    c = [np.float64(g[j]) + np.float64(a[j]) for j in (a01, a12, a23)]
    assert np.float64(0.0) + (c[0] + (c[1] + c[2])) == r["cutoff"]
    assert (c[0] + c[1]) + c[2] == np.nextafter(r["cutoff"], np.inf)


def test_plain_tool_restatement_scales_there_and_back():
    """--inv-acoustic-scale=12: acoustic values times float(1/12), pruned, times the DOUBLE 1 / float(1/12): 3 -> 0.25 -> 3,
    but 7 -> 0.5833334 -> 7.0000005 (0x1.c00002p+2: not the input's bits)."""
    c = latprune_cases.scaled_there_and_back()
    out = R.plain_tool(c, _api().compact_lattice_to_prune_csr(c), 1.0, 12.0, 4.0)
    assert out["ok"] and list(out["kept_arcs"]) == [0, 1] and list(out["arc_g"]) == [1.5, 2.0]
    there = np.float32(np.float64(np.float32(1.0) / np.float32(12.0)) * 7.0)
    back = np.float32(1.0 / np.float64(np.float32(1.0) / np.float32(12.0)) * np.float64(there))
    assert out["arc_a"][0] == np.float32(3.0) and out["arc_a"][1] == back and back == np.float32(float.fromhex("0x1.c00002p+2"))
    assert out["final_g"][1] == np.float32(0.5) and out["final_a"][1] == np.float32(6.0) and out["final_g"][0] == np.float32(np.inf)


# ---------------------------------------------------------------- the tool's logic that needs no device
LATS_TEXT = (b"utt1 \n"
             b"0\t1\t5\t1.5,3,7_8\n"
             b"1\t0.5,6,9\n"
             b"\n")


def _tool():
    return __import__("tools.lattice_prune", fromlist=["main"])


def test_tool_option_errors(tmp_path, capfd):
    """Usage: 1; a bad option or a zero scale: 255 (the binary's -1); both acoustic scales set (:59) or beam <= 0
    (PruneLattice :192): the assertion's abort, 134; a sweep with the plain scale options or with wspecifiers that do not
    differ per point is refused.  None of these reaches the device."""
    tool = _tool()
    src = tmp_path / "in.lats"
    src.write_bytes(LATS_TEXT)
    rs, ws = "ark:%s" % src, "ark:%s" % (tmp_path / "out.lats")
    assert tool.main([rs]) == 1
    assert "Usage: lattice-prune [options] lattice-rspecifier lattice-wspecifier" in capfd.readouterr().err
    assert tool.main([rs, ws, ws]) == 1
    assert tool.main(["--no-such-option=1", rs, ws]) == 255
    assert tool.main(["--acoustic-scale=0.5", "--inv-acoustic-scale=2", rs, ws]) == 134
    assert "acoustic_scale == 1.0 || inv_acoustic_scale == 1.0" in capfd.readouterr().err
    assert tool.main(["--acoustic-scale=0", rs, ws]) == 255
    assert "Do not use a zero acoustic scale (cannot be inverted)" in capfd.readouterr().err
    assert tool.main(["--beam=0", rs, ws]) == 134
    assert tool.main(["--beam=-1", "--inv-acoustic-scales=9:10", rs, "ark:%s" % (tmp_path / "LMWT.lats")]) == 134
    assert "beam > 0.0" in capfd.readouterr().err
    assert tool.main(["--inv-acoustic-scales=9:10", "--acoustic-scale=0.5", rs, "ark:%s" % (tmp_path / "LMWT.lats")]) == 255
    assert "do not combine it with --acoustic-scale / --inv-acoustic-scale" in capfd.readouterr().err
    assert tool.main(["--inv-acoustic-scales=9:10", "--inv-acoustic-scale=2", rs, "ark:%s" % (tmp_path / "LMWT.lats")]) == 255
    assert tool.main(["--inv-acoustic-scales=9:10", "--word-ins-penalties=0.0,0.5", rs, "ark:%s" % (tmp_path / "LMWT.lats")]) == 255
    assert "must differ per point" in capfd.readouterr().err
    assert tool.main(["--inv-acoustic-scales=9:10", rs, ws]) == 255
    assert tool.main(["--inv-acoustic-scales=10:9", rs, "ark:%s" % (tmp_path / "LMWT.lats")]) == 255
    assert not (tmp_path / "out.lats").exists() and not (tmp_path / "9.lats").exists()


def test_tool_scales_and_sweep_helpers():
    tool = _tool()
    assert tool.kt.parse_sweep_list("9:11", "x") == ["9", "10", "11"]
    assert tool.kt.substitute("ark:pruned/penalty_WIP/LMWT.lats", "12", "0.5") == "ark:pruned/penalty_0.5/12.lats"
    ac = tool.plain_scale(1.0, 12.0)
    assert ac.dtype == np.float32 and ac == np.float32(1.0) / np.float32(12.0)
    assert tool.plain_scale(0.1, 1.0) == np.float32(0.1)
    assert tool.acoustic_lattice_scale(ac).tolist() == [[1.0, 0.0], [0.0, float(ac)]]
    # the subset the tool writes: the kept states and arcs of the api's answer carrying another lattice's weights
    name, clat, _, _, want = latprune_cases.unsorted_start_not_zero()
    r = dict(ok=True, n_states=3, start=0, kept_states=np.array([2, 0, 3]), kept_arcs=np.array([0, 1]), arc_src=np.array([0, 1], np.int32),
             arc_dst=np.array([1, 2], np.int32), final_kept=np.array([False, False, True]))
    sub = tool.pruned_subset(clat, r)
    assert list(sub["arc_label"]) == [1, 2] and [list(x) for x in sub["arc_string"]] == [[21], [22]]
    assert list(sub["final_g"]) == [np.inf, np.inf, 0.0] and [list(x) for x in sub["final_string"]] == [[], [], [24]]
    assert tool.pruned_subset(clat, dict(ok=False))["n_states"] == 0


def test_bin_shim_is_executable():
    p = os.path.join(ROOT, "bin", "lattice-prune")
    assert os.access(p, os.X_OK) and "tools/lattice_prune.py" in open(p).read()


# ---------------------------------------------------------------- the entry points
def test_entry_points_declared_and_loud_without_a_device():
    import torch
    capi = pkg("capi")
    lib = capi.load()
    names = ("kh_compact_lattice_prune", "kh_compact_lattice_prune_set_workspace_limit", "kh_compact_lattice_prune_last_timings")
    header = open(os.path.join(ROOT, "include", "kaldi_hip.h")).read()
    for n in names:
        assert n in capi.SIGNATURES and hasattr(lib, n) and n + "(" in header
    api = _api()
    empty = pkg("kaldi_io").read_compact_lattice(__import__("io").BytesIO(b"\n"), binary=False)
    res = api.compact_lattice_prune([empty], [api.score_point()] * 2, 1.0)      # no start state: no device call
    assert [r["ok"] for r in res[0]] == [False, False] and res[0][0]["n_states"] == 0 and res[0][0]["start"] == -1
    if torch.cuda.is_available():
        return
    csr = api.compact_lattice_to_prune_csr(latprune_cases.tie_at_the_cutoff()[1])
    with pytest.raises(capi.KhError, match="no HIP device"):
        api.compact_lattice_prune_raw([csr], [0], [api.score_point()], 1.0)
