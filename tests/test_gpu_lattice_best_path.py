"""GPU box: kh_compact_lattice_best_paths (csrc/kh_latbest.hip) against the line-by-line restatement
(latbest_restatement.py).  Equality is exact everywhere - words, alignments, path arcs, the bit patterns of the float
totals: both sides perform the same IEEE operations in the same order with contraction off, so a tolerance would only hide
a wrong tie rule."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import latbest_cases
import latbest_restatement as R
from test_gpu_determinize import structured_case

pytestmark = pytest.mark.gpu


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def extra_points(api):
    """Off-diagonal scales and negative penalties."""
    return [(np.array([1.0, 0.25, -0.125, 0.5]), np.float32(-0.75)), (np.array([0.0, 1.0, 1.0, 0.0]), np.float32(0.25)),
            api.score_point(lm_scale=0.0, acoustic_scale=1.0, word_ins_penalty=-1.5), api.score_point(lm_scale=2.5, acoustic2lm_scale=0.1)]


def assert_same(got, want, what):
    if want is None or got is None:
        assert got is None and want is None, what
        return
    assert np.array_equal(got["words"], want["words"]), what
    assert np.array_equal(got["alignment"], want["alignment"]), what
    assert np.array_equal(got["arcs"], want["arcs"]) and got["final_state"] == want["final_state"], what
    assert bits(got["graph_cost"]) == bits(want["graph_cost"]) and bits(got["acoustic_cost"]) == bits(want["acoustic_cost"]), \
        (what, got["graph_cost"], want["graph_cost"], got["acoustic_cost"], want["acoustic_cost"])


def assert_batch_equals_restatement(api, clats, points, res):
    for i, c in enumerate(clats):
        csr = api.compact_lattice_to_csr(c)
        for p, (scale, pen) in enumerate(points):
            assert_same(res[i][p], R.best_path_of_clat(c, csr, scale, pen), (i, p))


def test_hand_lattices(api):
    """Every hand lattice alone and all of them in one batch, each with its own point and with all points at once."""
    cases = latbest_cases.all_cases()
    for name, clat, point, want in cases:
        latbest_cases.check_result(api.compact_lattice_best_paths([clat], [point])[0][0], want, name)
    points = [c[2] for c in cases]
    res = api.compact_lattice_best_paths([c[1] for c in cases], points)
    for i, (name, clat, point, want) in enumerate(cases):
        latbest_cases.check_result(res[i][i], want, name)
    assert_batch_equals_restatement(api, [c[1] for c in cases], points, res)


def test_unsorted_csr_is_refused(api):
    """The C entry point takes top-sorted lattices only: KH_EINVAL, with the arc named."""
    capi = importlib.import_module("old-kaldi-git_amd.capi")
    csr = api.compact_lattice_to_csr(latbest_cases.predecessor_tie()[1])
    bad = dict(csr, arc_nextstate=np.array([1, 2, 3, 1], np.int32))
    with pytest.raises(capi.KhError, match="topologically sorted"):
        api.compact_lattice_best_paths_raw([bad], [api.score_point()])


def fuzz_lattices():
    """240 seeded lattices, 2 ... 3000 states (most small, every eighth large); every one has its last state final and
    reachable from every state, so every one has a path."""
    out = []
    for seed in range(240):
        rng = np.random.default_rng(7000 + seed)
        n = int(rng.integers(500, 3001)) if seed % 8 == 0 else int(rng.integers(2, 120))
        out.append(R.random_clat(rng, n, max_out=int(rng.integers(1, 6)), quantum=0.25, p_eps=float(rng.choice([0.0, 0.2, 0.6])),
                                 p_final=float(rng.choice([0.0, 0.1]))))
    return out


def test_fuzz_against_the_restatement(api):
    """Weights are multiples of 0.25, so ties are the rule; the 36 points of the scoring scripts plus off-diagonal scales
    and negative penalties.  Every (lattice, point) pair is searched by the restatement on the CPU: all of them yield a
    path there, nothing is sampled, skipped or filtered, and the device's answer equals each exactly."""
    clats = fuzz_lattices()
    assert len(clats) >= 200 and max(c["n_states"] for c in clats) >= 2000
    points = R.score_points_36(api) + extra_points(api)
    wants = []
    for c in clats:
        csr = api.compact_lattice_to_csr(c)
        wants.append([R.best_path_of_clat(c, csr, scale, pen) for scale, pen in points])
        assert all(w is not None for w in wants[-1])
    res = api.compact_lattice_best_paths(clats, points)
    for i in range(len(clats)):
        for p in range(len(points)):
            assert_same(res[i][p], wants[i][p], (i, p))


def test_point_counts_and_bounded_workspace(api):
    """K = 1, 36, 64, 65 (a second wave per lattice) and a workspace limit that lets only a few lattices fly at once: the
    same answers point by point."""
    clats = fuzz_lattices()[:48]
    base = R.score_points_36(api) + extra_points(api)
    points = (base * 2)[:65]
    full = api.compact_lattice_best_paths(clats, points)
    assert api.compact_lattice_best_paths_last_timings()["launches"] == 1
    assert_batch_equals_restatement(api, clats[1:8], points[60:65], [r[60:65] for r in full[1:8]])
    for K in (1, 36, 64):
        part = api.compact_lattice_best_paths(clats, points[:K])
        for i in range(len(clats)):
            for p in range(K):
                assert_same(part[i][p], full[i][p], (K, i, p))
    biggest = max(c["n_states"] for c in clats)
    limit = biggest * 12 * 65              # less than the largest lattice alone needs (it still runs, alone)
    tight = api.compact_lattice_best_paths(clats, points, workspace_limit=limit)
    assert api.compact_lattice_best_paths_last_timings()["launches"] >= 2      # the batch did not fit at once
    for i in range(len(clats)):
        for p in range(65):
            assert_same(tight[i][p], full[i][p], ("tight", i, p))
    api.compact_lattice_best_paths(clats[:2], points[:1])
    assert api.compact_lattice_best_paths_last_timings()["launches"] == 1      # the limit did not stick
    # the limit belongs to the thread that set it
    import threading
    lib = importlib.import_module("old-kaldi-git_amd.capi").load()
    th = threading.Thread(target=lambda: lib.kh_compact_lattice_best_paths_set_workspace_limit(limit))
    th.start()
    th.join()
    api.compact_lattice_best_paths(clats, points)
    assert api.compact_lattice_best_paths_last_timings()["launches"] == 1


@pytest.fixture(scope="module")
def decoded_clats(api):
    """The CompactLattices of a small structured decode + determinization, as test_gpu_determinize.py obtains them."""
    g, tp, lls = structured_case(303, 200_000, 600, [120, 70, 33, 150])
    cfg = api.decoder_config(beam=13.0, max_active=2000, min_active=200, lattice_beam=7.0)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lls])]).astype(np.int32)
    dec = api.LatticeFasterDecoder(api.Fst(g), cfg, max_batch=len(lls), max_frames=max(len(x) for x in lls))
    dec.set_determinize(True, cfg["lattice_beam"], tid_phone=tp)
    dec.decode(torch.from_numpy(np.concatenate(lls)).cuda(), off)
    clats = [dec.get_compact_lattice(u) for u in range(len(lls))]
    assert all(c["complete"] and len(c["arc_src"]) > 0 for c in clats)
    return clats, [len(x) for x in lls]


def test_real_lattices(api, decoded_clats):
    """36 points in one call == 36 calls of one point == the restatement; every alignment has one transition-id per frame."""
    clats, lens = decoded_clats
    points = R.score_points_36(api)
    res = api.compact_lattice_best_paths(clats, points)
    for p, pt in enumerate(points):
        one = api.compact_lattice_best_paths(clats, [pt])
        for i in range(len(clats)):
            assert_same(one[i][0], res[i][p], (i, p))
    assert_batch_equals_restatement(api, clats, points, res)
    for i, T in enumerate(lens):
        assert all(len(r["alignment"]) == T for r in res[i])


def tool_written_archive(tmp_path, monkeypatch):
    """exp/decode/lat.1.gz and lat.2.gz written by this project's nnet-latgen-faster with the recipe's wspecifier
    ("ark:|gzip -c > lat.JOB.gz"), set up as tests/test_gpu_latgen_tool.py sets it up.  Returns the number of utterances."""
    from conftest import pkg
    kio, workloads = pkg("kaldi_io"), pkg("workloads")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import nnet_latgen_faster as tool
    n_pdf, acwt = 5, 0.2
    rng = np.random.default_rng(22)
    topo = dict(phones=list(range(1, n_pdf + 1)), phone2idx=[-1] + [0] * n_pdf, entries=[[(0, [(0, 0.5), (1, 0.5)]), (-1, [])]])
    pdf_of_phone = rng.permutation(n_pdf)
    triples = [(p + 1, 0, int(pdf_of_phone[p])) for p in range(n_pdf)]
    log_probs = np.concatenate([[0.0], np.full(2 * n_pdf, np.log(0.5))]).astype(np.float32)
    g = workloads.make_hclg_like(rng, 400, n_pdf, final_frac=0.2)
    g["tid2pdf"] = np.concatenate([[-1], np.repeat(pdf_of_phone, 2)]).astype(np.int32)
    monkeypatch.chdir(tmp_path)
    os.makedirs("exp/decode/scoring")
    os.makedirs("graph")
    with open("final.mdl", "wb") as f:
        f.write(b"\0B")
        kio.write_transition_model(f, topo, triples, log_probs, True)
        f.write(open(os.path.join(ROOT, "tests", "golden", "kaldi_io", "am_nnet_body_bin"), "rb").read())
    with open("graph/HCLG.fst", "wb") as f:
        kio.write_fst(f, g)
    with open("graph/words.txt", "w") as f:
        f.write("<eps> 0\n" + "".join("W%d %d\n" % (i, i) for i in range(1, int(g["olabel"].max()) + 1)))
    n = 0
    for job, lens in ((1, (37, 5, 64)), (2, (80, 23))):
        with kio.TableWriter("feats.%d.ark" % job) as w:
            for i, T in enumerate(lens):
                w.write("spk%d-utt%d" % (job, i), rng.standard_normal((T, 6)).astype(np.float32))
                n += 1
        assert tool.main(["--max-active=300", "--min-active=200", "--beam=9", "--lattice-beam=5", "--acoustic-scale=%g" % acwt,
                          "--allow-partial=true", "final.mdl", "graph/HCLG.fst", "ark:feats.%d.ark" % job,
                          "ark:|gzip -c > exp/decode/lat.%d.gz" % job]) == 0
    return n


def test_sweep_equals_the_three_programs_piped(api, tmp_path, monkeypatch):
    """local/score.sh's line - lattice-scale --inv-acoustic-scale=LMWT "ark:gunzip -c $dir/lat.*.gz|" ark:- |
    lattice-add-penalty --word-ins-penalty=$wip ark:- ark:- | lattice-best-path --word-symbol-table=$symtab ark:- ark,t:... -
    run through real pipes with bin/ first in PATH, once per (LMWT, wip) of the 12 x 3 grid, on archives written by this
    project's nnet-latgen-faster, against ONE lattice-best-path sweep reading the same rspecifier: the 36 .tra files (text)
    and the 36 alignment archives (binary) byte for byte.  The flipped formats (binary words, text alignments) are compared
    on the three penalties at LMWT 12, and what the files hold against the api."""
    cli = importlib.import_module("old-kaldi-git_amd.kaldi_cli")
    n_utts = tool_written_archive(tmp_path, monkeypatch)
    lats = "ark:gunzip -c exp/decode/lat.*.gz|"
    bp = importlib.import_module("tools.lattice_best_path")
    for wip in ("0.0", "0.5", "1.0"):
        os.makedirs("exp/decode/scoring/penalty_" + wip)
        os.makedirs("pipe/penalty_" + wip)
    assert bp.main(["--inv-acoustic-scales=9:20", "--word-ins-penalties=0.0,0.5,1.0", lats,
                    "ark,t:exp/decode/scoring/penalty_WIP/LMWT.tra", "ark:exp/decode/scoring/penalty_WIP/LMWT.ali"]) == 0
    assert bp.main(["--inv-acoustic-scales=12", "--word-ins-penalties=0.0,0.5,1.0", lats,
                    "ark:exp/decode/scoring/penalty_WIP/LMWT.btra", "ark,t:exp/decode/scoring/penalty_WIP/LMWT.tali"]) == 0
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)

    def pipe(lmwt, wip, tra, ali):
        cmd = ('lattice-scale --inv-acoustic-scale=%s "%s" ark:- | lattice-add-penalty --word-ins-penalty=%s ark:- ark:- | '
               'lattice-best-path --word-symbol-table=graph/words.txt ark:- %s %s' % (lmwt, lats, wip, tra, ali))
        r = subprocess.run(["sh", "-c", cmd], env=env, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert b"Done %d lattices, failed for 0" % n_utts in r.stderr and b"spk2-utt1 " in r.stderr
    for wip in ("0.0", "0.5", "1.0"):
        for lmwt in range(9, 21):
            d, s = "pipe/penalty_%s/%d" % (wip, lmwt), "exp/decode/scoring/penalty_%s/%d" % (wip, lmwt)
            pipe(lmwt, wip, "ark,t:%s.tra" % d, "ark:%s.ali" % d)
            for ext in (".tra", ".ali"):
                want, got = open(d + ext, "rb").read(), open(s + ext, "rb").read()
                assert len(want) > 0 and got == want, (wip, lmwt, ext)
        d, s = "pipe/penalty_%s/12" % wip, "exp/decode/scoring/penalty_%s/12" % wip
        pipe(12, wip, "ark:%s.btra" % d, "ark,t:%s.tali" % d)
        for ext in (".btra", ".tali"):
            assert open(d + ext, "rb").read() == open(s + ext, "rb").read(), (wip, ext)
    # ... and what the files hold is what the api returns
    import gzip
    kio = importlib.import_module("old-kaldi-git_amd.kaldi_io")
    clats = [kv for job in (1, 2) for kv in kio.read_ark(gzip.open("exp/decode/lat.%d.gz" % job), kind="compact_lattice")]
    assert len(clats) == n_utts
    res = api.compact_lattice_best_paths([c for _, c in clats], [api.score_point(inv_acoustic_scale=12.0, word_ins_penalty=0.5)])
    tra = dict(cli.SequentialTableReader("ark:exp/decode/scoring/penalty_0.5/12.tra", "int32_vector"))
    ali = dict(cli.SequentialTableReader("ark:exp/decode/scoring/penalty_0.5/12.ali", "int32_vector"))
    for (key, _), row in zip(clats, res):
        assert np.array_equal(tra[key], row[0]["words"]) and np.array_equal(ali[key], row[0]["alignment"])


def test_plain_tool_options_and_failure(api, decoded_clats, tmp_path, capfd):
    """lattice-best-path without the sweep: --acoustic-scale / --lm-scale as LatticeScale(lm_scale, acoustic_scale), the
    per-utterance and closing log lines, the symbol table's debug output; a lattice without a final state counts as a
    failure and writes nothing; an archive of such lattices alone gives exit status 1."""
    cli = importlib.import_module("old-kaldi-git_amd.kaldi_cli")
    bp = importlib.import_module("tools.lattice_best_path")
    clats, lens = decoded_clats
    lats, bad, tra = tmp_path / "lat.1", tmp_path / "bad.lats", tmp_path / "out.tra"
    w = cli.TableWriter("ark:%s" % lats, "compact_lattice")
    w.write("utt00", clats[0])
    w.write("nofinal", latbest_cases.no_final_state()[1])
    w.write("hand", latbest_cases.penalty_zero()[1])
    w.close()
    syms = tmp_path / "words.txt"
    syms.write_text("<eps> 0\n" + "".join("w%d %d\n" % (k, k) for k in range(1, int(clats[0]["arc_label"].max()) + 3)))
    assert bp.main(["--acoustic-scale=0.1", "--lm-scale=0.5", "--word-symbol-table=%s" % syms, "ark:%s" % lats, "ark,t:%s" % tra]) == 0
    err = capfd.readouterr().err
    want = api.compact_lattice_best_paths([clats[0]], [api.score_point(lm_scale=0.5, acoustic_scale=0.1)])[0][0]
    lines = tra.read_bytes().splitlines()
    assert lines == [b"utt00 " + b"".join(b"%d " % x for x in want["words"]), b"hand 1 2 "]
    assert "For utterance utt00, best cost" in err and "over %d frames." % lens[0] in err
    assert "For utterance hand, best cost 0.5 + 0 = 0.5 over 2 frames." in err
    assert "Best-path failed for key nofinal" in err and "hand w1 w2 \n" in err
    assert "Done 2 lattices, failed for 1" in err and "Overall score per frame is" in err
    w = cli.TableWriter("ark:%s" % bad, "compact_lattice")
    w.write("nofinal", latbest_cases.no_final_state()[1])
    w.close()
    assert bp.main(["ark:%s" % bad, "ark,t:%s" % tra]) == 1
    assert tra.read_bytes() == b""
