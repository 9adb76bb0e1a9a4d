"""GPU box: kh_compact_lattice_prune (csrc/kh_latprune.hip) against the line-by-line restatement (latprune_restatement.py).
Equality is exact everywhere - masks, state numbering, arc order, the bit patterns of the floats: both sides perform the
same IEEE operations in the same association with contraction off, so a tolerance would only hide a wrong comparison."""
import importlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from conftest import ROOT

import latprune_cases
import latprune_restatement as R
from latbest_restatement import score_points_36
from test_gpu_determinize import structured_case

pytestmark = pytest.mark.gpu

BEAMS = (0.25, 1.0, 2.5, 4.0, 6.0)


def extra_points(api):
    """The off-diagonal scales and negative penalties of the best-path test."""
    return [(np.array([1.0, 0.25, -0.125, 0.5]), np.float32(-0.75)), (np.array([0.0, 1.0, 1.0, 0.0]), np.float32(0.25)),
            api.score_point(lm_scale=0.0, acoustic_scale=1.0, word_ins_penalty=-1.5), api.score_point(lm_scale=2.5, acoustic2lm_scale=0.1)]


def assert_raw_equals(raw, i, p, r, what, q=None):
    """Lattice i, point p of compact_lattice_prune_raw's answer against prune_lattice's r."""
    s0, s1, a0, a1 = raw["state_offsets"][i], raw["state_offsets"][i + 1], raw["arc_offsets"][i], raw["arc_offsets"][i + 1]
    assert np.array_equal(raw["arc_keep"][a0:a1, p], r["arc_keep"]), what
    assert np.array_equal(raw["state_keep"][s0:s1, p], r["state_keep"]), what
    assert np.array_equal(raw["final_keep"][s0:s1, p], r["final_keep"]), what
    assert np.float64(raw["best_final_cost"][i, p]).view(np.int64) == np.float64(r["best_final_cost"]).view(np.int64), what


def test_hand_lattices(api):
    """Every hand lattice alone, and all of them in one batch with a point (and a beam) each."""
    cases = latprune_cases.all_cases()
    for name, clat, point, beam, want in cases:
        got = api.compact_lattice_prune([clat], [point], beam)[0][0]
        latprune_cases.check_result(got, want, name, clat)
        R.assert_same_clat(got, R.prune_clat(clat, api.compact_lattice_to_prune_csr(clat), point[0], point[1], beam), name)
        raw = api.compact_lattice_prune_raw([api.compact_lattice_to_prune_csr(clat)], [api.compact_lattice_to_prune_csr(clat)["start"]],
                                            [point], beam)
        assert raw["best_final_cost"][0, 0] == want["best_final_cost"], name
    points, beams = [c[2] for c in cases], [c[3] for c in cases]
    res = api.compact_lattice_prune([c[1] for c in cases], points, beams)
    for i, (name, clat, point, beam, want) in enumerate(cases):
        latprune_cases.check_result(res[i][i], want, name, clat)
        csr = api.compact_lattice_to_prune_csr(clat)
        for p, (pt, b) in enumerate(zip(points, beams)):
            R.assert_same_clat(res[i][p], R.prune_clat(clat, csr, pt[0], pt[1], b), (name, p))


@pytest.fixture(scope="module")
def fuzz(api):
    """120 seeded lattices, most with 2 ... 120 states, every twelfth with 500 ... 3000 (one of them made >= 2000); the 36
    points of the scoring grid plus off-diagonal scales and negative penalties, the beams cycling; the restatement's answer
    for every (lattice, point) pair, computed once."""
    clats = []
    for seed in range(120):
        rng = np.random.default_rng(11000 + seed)
        n = int(rng.integers(500, 3001)) if seed % 12 == 0 else int(rng.integers(2, 121))
        if seed == 24:
            n = max(n, 2000)
        clats.append(R.random_clat(rng, n, max_out=int(rng.integers(1, 6)), quantum=0.25, p_eps=float(rng.choice([0.0, 0.2, 0.6])),
                                   p_final=float(rng.choice([0.0, 0.1]))))
    points = score_points_36(api) + extra_points(api)
    beams = [BEAMS[p % len(BEAMS)] for p in range(len(points))]
    csrs = [api.compact_lattice_to_prune_csr(c) for c in clats]
    wants = [[R.prune_lattice(csr, pt[0], pt[1], b) for pt, b in zip(points, beams)] for csr in csrs]
    return clats, csrs, points, beams, wants


def test_fuzz_against_the_restatement(api, fuzz):
    """Weights are multiples of 0.25, so ties at the cutoff are common.  Every (lattice, point) pair equals the restatement:
    the raw masks and best_final_cost, and the assembled CompactLattice.  Nothing is sampled, skipped or filtered.  The
    conditions on the cases are asserted on the restatement's answers only."""
    clats, csrs, points, beams, wants = fuzz
    assert len(clats) == 120 and max(c["n_states"] for c in clats) >= 2000 and len(points) == 40
    n_pairs = len(clats) * len(points)
    assert all(r["state_keep"].any() for row in wants for r in row)            # no pair is empty
    busy = sum(1 for row in wants for r in row if not r["arc_keep"].all() and r["state_keep"].any())
    print("pairs with an arc removed and a state kept: %d of %d" % (busy, n_pairs))
    assert busy >= 0.9 * n_pairs
    raw = api.compact_lattice_prune_raw(csrs, [c["start"] for c in csrs], points, beams)
    for i in range(len(clats)):
        for p in range(len(points)):
            assert_raw_equals(raw, i, p, wants[i][p], (i, p))
    res = api.compact_lattice_prune(clats, points, beams)
    for i, (c, csr) in enumerate(zip(clats, csrs)):
        for p in range(len(points)):
            r = wants[i][p]
            R.assert_same_clat(res[i][p], R._subset(c, csr, r, *r["weights"]), (i, p))


def test_point_counts_and_bounded_workspace(api, fuzz):
    """K = 1, 36, 64, 65 (a second mask word and a second wave per lattice) and a workspace limit that lets only a few
    lattices fly at once: the same answers point by point (point p of the doubled list is point p % 40 of the fuzz, with
    the same beam: 40 is a multiple of the beams' cycle)."""
    clats, csrs, points, beams, wants = fuzz
    sub = csrs[:26]                       # with the large lattices of seeds 0, 12 and 24
    starts = [c["start"] for c in sub]
    pts, bms = (points * 2)[:65], (beams * 2)[:65]
    for K in (65, 1, 36, 64):
        raw = api.compact_lattice_prune_raw(sub, starts, pts[:K], bms[:K])
        assert api.compact_lattice_prune_last_timings()["launches"] == 1
        assert raw["arc_keep"].shape[1] == K
        for i in range(len(sub)):
            for p in range(K):
                assert_raw_equals(raw, i, p, wants[i][p % 40], (K, i, p))
    biggest = max(c["n_states"] for c in sub)
    limit = biggest * 8 * 128 - 1         # less than the largest lattice alone needs at two mask words (it still runs, alone)
    tight = api.compact_lattice_prune_raw(sub, starts, pts, bms, workspace_limit=limit)
    assert api.compact_lattice_prune_last_timings()["launches"] >= 2
    for i in range(len(sub)):
        for p in range(65):
            assert_raw_equals(tight, i, p, wants[i][p % 40], ("tight", i, p))
    api.compact_lattice_prune_raw(sub, starts, pts, bms)
    assert api.compact_lattice_prune_last_timings()["launches"] == 1      # the limit did not stick
    lib = importlib.import_module("old-kaldi-git_amd.capi").load()
    th = threading.Thread(target=lambda: lib.kh_compact_lattice_prune_set_workspace_limit(limit))
    th.start()
    th.join()
    api.compact_lattice_prune_raw(sub, starts, pts, bms)
    assert api.compact_lattice_prune_last_timings()["launches"] == 1      # ... and belongs to the thread that set it


def test_refusals(api):
    """KH_EINVAL with the offender named."""
    capi = importlib.import_module("old-kaldi-git_amd.capi")
    csr = api.compact_lattice_to_prune_csr(latprune_cases.tie_at_the_cutoff()[1])
    pt = [api.score_point()]
    with pytest.raises(capi.KhError, match=r"arc 1 \(state 0 -> 0 of 3\).*topologically sorted"):
        api.compact_lattice_prune_raw([dict(csr, arc_nextstate=np.array([1, 0, 2, 2], np.int32))], [0], pt, 1.0)
    for bad in (3, -1):
        with pytest.raises(capi.KhError, match="start state %d of 3 states" % bad):
            api.compact_lattice_prune_raw([csr], [bad], pt, 1.0)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(capi.KhError, match="point 1: beam"):
            api.compact_lattice_prune_raw([csr], [0], pt * 2, [1.0, bad])
    g = csr["arc_graph"].copy()
    g[2] = np.nan
    with pytest.raises(capi.KhError, match=r"arc 2 \(state 0 -> 2\).*NaN"):
        api.compact_lattice_prune_raw([dict(csr, arc_graph=g)], [0], pt, 1.0)
    fa = csr["final_acoustic"].copy()
    fa[1] = -np.inf
    with pytest.raises(capi.KhError, match="state 1: final weight"):
        api.compact_lattice_prune_raw([dict(csr, final_acoustic=fa)], [0], pt, 1.0)
    with pytest.raises(capi.KhError):
        api.compact_lattice_prune_raw([csr], [0], [], 1.0)


@pytest.fixture(scope="module")
def decoded_clats(api):
    """The CompactLattices of a small structured decode + determinization, as test_gpu_lattice_best_path.py obtains them."""
    g, tp, lls = structured_case(303, 200_000, 600, [120, 70, 33, 150])
    cfg = api.decoder_config(beam=13.0, max_active=2000, min_active=200, lattice_beam=7.0)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lls])]).astype(np.int32)
    dec = api.LatticeFasterDecoder(api.Fst(g), cfg, max_batch=len(lls), max_frames=max(len(x) for x in lls))
    dec.set_determinize(True, cfg["lattice_beam"], tid_phone=tp)
    dec.decode(torch.from_numpy(np.concatenate(lls)).cuda(), off)
    clats = [dec.get_compact_lattice(u) for u in range(len(lls))]
    assert all(c["complete"] and len(c["arc_src"]) > 0 for c in clats)
    return clats


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def test_real_lattices(api, decoded_clats):
    """All grid points at beam 5 equal the restatement; the best path survives the pruning: words, alignment and the
    cost's bits at the identity point are those of the unpruned lattice."""
    clats = decoded_clats
    points = score_points_36(api)
    res = api.compact_lattice_prune(clats, points, 5.0)
    for i, c in enumerate(clats):
        csr = api.compact_lattice_to_prune_csr(c)
        for p, (scale, pen) in enumerate(points):
            R.assert_same_clat(res[i][p], R.prune_clat(c, csr, scale, pen, 5.0), (i, p))
    ident = [api.score_point()]
    pruned = [row[0] for row in api.compact_lattice_prune(clats, ident, 5.0)]
    assert all(q["ok"] for q in pruned)
    assert sum(len(q["arc_src"]) for q in pruned) < sum(len(c["arc_src"]) for c in clats)
    before, after = api.compact_lattice_best_paths(clats, ident), api.compact_lattice_best_paths(pruned, ident)
    for i in range(len(clats)):
        b, a = before[i][0], after[i][0]
        assert np.array_equal(a["words"], b["words"]) and np.array_equal(a["alignment"], b["alignment"]), i
        assert bits(a["graph_cost"]) == bits(b["graph_cost"]) and bits(a["acoustic_cost"]) == bits(b["acoustic_cost"]), i


def test_sweep_equals_the_three_programs_piped(api, decoded_clats, tmp_path, monkeypatch):
    """lattice-scale --inv-acoustic-scale=LMWT | lattice-add-penalty --word-ins-penalty=$wip | lattice-prune --beam=5 run
    through real pipes with bin/ first in PATH, once per point, against ONE lattice-prune sweep reading the same archive:
    the files byte for byte, binary for every point and text (ark,t) for two of them."""
    cli = importlib.import_module("old-kaldi-git_amd.kaldi_cli")
    tool = importlib.import_module("tools.lattice_prune")
    monkeypatch.chdir(tmp_path)
    w = cli.TableWriter("ark:lats.ark", "compact_lattice")
    for i, c in enumerate(decoded_clats):
        w.write("utt%02d" % i, c)
    w.write("hand", latprune_cases.tie_at_the_cutoff()[1])
    w.close()
    for wip in ("0.0", "0.5"):
        os.makedirs("sweep/penalty_" + wip)
        os.makedirs("pipe/penalty_" + wip)
    assert tool.main(["--inv-acoustic-scales=9,12", "--word-ins-penalties=0.0,0.5", "--beam=5", "ark:lats.ark",
                      "ark:sweep/penalty_WIP/LMWT.lats"]) == 0
    assert tool.main(["--inv-acoustic-scales=12", "--word-ins-penalties=0.0,0.5", "--beam=5", "ark:lats.ark",
                      "ark,t:sweep/penalty_WIP/LMWT.txt"]) == 0
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)

    def pipe(lmwt, wip, wspec):
        cmd = ("lattice-scale --inv-acoustic-scale=%s ark:lats.ark ark:- | lattice-add-penalty --word-ins-penalty=%s ark:- ark:- | "
               "lattice-prune --beam=5 ark:- %s" % (lmwt, wip, wspec))
        r = subprocess.run(["sh", "-c", cmd], env=env, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert b"Done %d lattices." % (len(decoded_clats) + 1) in r.stderr
    for wip in ("0.0", "0.5"):
        for lmwt in ("9", "12"):
            pipe(lmwt, wip, "ark:pipe/penalty_%s/%s.lats" % (wip, lmwt))
            want, got = (open("%s/penalty_%s/%s.lats" % (d, wip, lmwt), "rb").read() for d in ("pipe", "sweep"))
            assert len(want) > 0 and got == want, (wip, lmwt)
        pipe("12", wip, "ark,t:pipe/penalty_%s/12.txt" % wip)
        want, got = (open("%s/penalty_%s/12.txt" % (d, wip), "rb").read() for d in ("pipe", "sweep"))
        assert len(want) > 0 and got == want, (wip, "text")
    # ... and what the files hold is what the api returns
    res = api.compact_lattice_prune(decoded_clats, [api.score_point(inv_acoustic_scale=12.0, word_ins_penalty=0.5)], 5.0)
    back = dict(cli.SequentialTableReader("ark:sweep/penalty_0.5/12.lats", "compact_lattice"))
    for i, row in enumerate(res):
        f = back["utt%02d" % i]
        assert f["n_states"] == row[0]["n_states"] and np.array_equal(f["arc_dst"], row[0]["arc_dst"])
        assert np.array_equal(bits(f["arc_g"]), bits(row[0]["arc_g"])) and np.array_equal(bits(f["arc_a"]), bits(row[0]["arc_a"]))


def test_plain_tool(api, decoded_clats, tmp_path, capfd):
    """lattice-prune --inv-acoustic-scale=12 --beam=4: the archive equals the restatement's scale / prune / scale-back
    written by write_compact_lattice; the log lines; a lattice that prunes to nothing is still written, with a warning,
    and the exit status stays 0; an empty archive gives 1."""
    cli = importlib.import_module("old-kaldi-git_amd.kaldi_cli")
    tool = importlib.import_module("tools.lattice_prune")
    clats = list(decoded_clats[:2]) + [latprune_cases.unsorted_start_not_zero()[1], latprune_cases.no_reachable_final()[1],
                                       latprune_cases.scaled_there_and_back()]
    keys = ["utt00", "utt01", "hand", "nofinal", "thereback"]
    src, out, want = tmp_path / "in.lats", tmp_path / "out.lats", tmp_path / "want.lats"
    w = cli.TableWriter("ark:%s" % src, "compact_lattice")
    for k, c in zip(keys, clats):
        w.write(k, c)
    w.close()
    assert tool.main(["--inv-acoustic-scale=12", "--beam=4", "ark:%s" % src, "ark:%s" % out]) == 0
    err = capfd.readouterr().err
    wants = [R.plain_tool(c, api.compact_lattice_to_prune_csr(c), 1.0, 12.0, 4.0) for c in clats]
    w = cli.TableWriter("ark:%s" % want, "compact_lattice")
    for k, x in zip(keys, wants):
        w.write(k, x)
    w.close()
    assert out.read_bytes() == want.read_bytes() and len(out.read_bytes()) > 0
    assert [x["ok"] for x in wants] == [True, True, True, False, True]
    # 7 -> 0.5833334 -> 7.0000005: what is written is not the input's bits (the decoded lattices' values may all come back)
    assert list(wants[4]["kept_arcs"]) == [0, 1] and np.any(bits(wants[4]["arc_a"]) != bits(np.asarray(clats[4]["arc_a"])[:2]))
    for k, c, x in zip(keys, clats, wants):
        assert ("For utterance %s, pruned #states from %d to %d and #arcs from %d to %d"
                % (k, c["n_states"], x["n_states"], len(c["arc_src"]), len(x["arc_src"]))) in err
    assert "WARNING (lattice-prune:main()) Error pruning lattice for utterance nofinal" in err
    assert "Overall, pruned from on average" in err and "over 5 utterances." in err and "Done 5 lattices." in err
    # one lattice that prunes to nothing: the key is written, exit status 0
    w = cli.TableWriter("ark:%s" % src, "compact_lattice")
    w.write("nofinal", clats[3])
    w.close()
    assert tool.main(["ark:%s" % src, "ark,t:%s" % out]) == 0
    assert out.read_bytes() == b"nofinal \n\n" and "Error pruning lattice for utterance nofinal" in capfd.readouterr().err
    src.write_bytes(b"")
    assert tool.main(["ark:%s" % src, "ark,t:%s" % out]) == 1
    assert out.read_bytes() == b"" and "Done 0 lattices." in capfd.readouterr().err
