"""GPU: stage 4 of steps/decode_fmllr.sh on files, literally and through the bin/ shims only -

  gmm-latgen-faster --determinize-lattice=false ... "ark:|gzip -c > lat.tmp.gz"
  gmm-rescore-lattice final.mdl "ark:gunzip -c lat.tmp.gz|" "ark,s,cs:... transform-feats --utt2spk=... |" ark:- | \\
    lattice-determinize-pruned --acoustic-scale=0.083333 --beam=6.0 ark:- "ark:|gzip -c > lat.gz"

- with the rescored table held to api.gmm_rescore_compact_lattices and the determinized one to api.determinize_lattice_pruned
on the same inputs, byte for byte; then --old-acoustic-scale, a missing feature key and the closing lines in process."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import fmllr_cases as FC
import rescore_restatement as R
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32
KEYS = ["utt0", "utt1", "utt2"]
SPAN = {"utt0": (0, 60), "utt1": (470, 525), "utt2": (670, 715)}      # frames of the fMLLR case: speaker A, speaker B twice
UTT2SPK = {"utt0": "spkA", "utt1": "spkB", "utt2": "spkB"}
TF = "transform-feats --utt2spk=ark:utt2spk ark:trans.ark"


def tool(name):
    return importlib.import_module(name.replace("-", "_"))


def shim_env():
    return dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)


def shell(d, cmd, want=0):
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=d, env=shim_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == want, p.stderr[-3000:]
    return p.stderr


def read_table(path, kind):
    return list(pkg("kaldi_cli").SequentialTableReader("ark:%s" % path, kind))


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle, api):
    """final.mdl, HCLG.fst, feats.ark (3 utterances, 2 speakers), utt2spk, trans.ark (an affine transform per speaker), and
    what the first two commands of the stage leave: lat.tmp.gz (state-level lattices) and, through the literal pipe, lat.gz."""
    cli, kio, workloads = pkg("kaldi_cli"), pkg("kaldi_io"), pkg("workloads")
    d = tmp_path_factory.mktemp("rescore")
    am, feats, _, _, _, _ = FC.e2e_case(oracle)
    FC.e2e_model_files(kio, am, str(d / "final.mdl"))
    rng = np.random.default_rng(41)
    g = workloads.make_hclg_like(rng, 300, 6, final_frac=0.2)
    g["tid2pdf"] = np.concatenate([[-1], np.repeat(np.arange(6), 2)]).astype(np.int32)
    with open(d / "HCLG.fst", "wb") as f:
        kio.write_fst(f, g)
    w = cli.TableWriter("ark:" + str(d / "feats.ark"), "matrix")
    for k in KEYS:
        w.write(k, feats[SPAN[k][0]:SPAN[k][1]])
    w.close()
    with open(d / "utt2spk", "w") as f:
        for k in KEYS:
            f.write("%s %s\n" % (k, UTT2SPK[k]))
    w = cli.TableWriter("ark:" + str(d / "trans.ark"), "matrix")
    for s in ("spkA", "spkB"):
        w.write(s, (np.eye(13, 14) + 0.05 * rng.standard_normal((13, 14))).astype(F))
    w.close()
    opts = "--beam=10 --max-active=200 --lattice-beam=6 --acoustic-scale=0.083333 --allow-partial=true --determinize-lattice=false"
    feats_pipe = "ark,s,cs:cat feats.ark | %s ark:- ark:- |" % TF
    shell(d, "gmm-latgen-faster %s final.mdl HCLG.fst '%s' 'ark:|gzip -c > lat.tmp.gz'" % (opts, feats_pipe))
    err = shell(d, "gmm-rescore-lattice final.mdl 'ark:gunzip -c lat.tmp.gz|' '%s' ark:- | "
                "lattice-determinize-pruned --acoustic-scale=0.083333 --beam=6.0 ark:- 'ark:|gzip -c > lat.gz'" % feats_pipe)
    shell(d, "gunzip -c lat.tmp.gz > lat.tmp.ark && gunzip -c lat.gz > lat.ark")
    return dict(dir=d, pipe_err=err)


@pytest.fixture(scope="module")
def in_process(files, api):
    """The same two steps from the library calls: the adapted features (transform-feats to a file), the model as the tool
    builds it, api.gmm_rescore_compact_lattices on the converted lattices with their old scores scaled by 0.0."""
    import torch
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    d = files["dir"]
    cwd = os.getcwd()
    os.chdir(d)
    try:
        assert tool("transform-feats").main(["--utt2spk=ark:utt2spk", "ark:trans.ark", "ark:feats.ark", "ark:adapted.ark"]) == 0
        assert tool("gmm-rescore-lattice").main(["final.mdl", "ark:lat.tmp.ark", "ark:adapted.ark", "ark:resc.ark"]) == 0
    finally:
        os.chdir(cwd)
    tm, am = cli.read_kaldi_object(str(d / "final.mdl"), lambda s, b: (kio.read_transition_model(s, b), kio.read_am_diag_gmm(s, b)))
    gconsts, _ = api.gmm_compute_gconsts(am["weights"], am["means_invvars"], am["inv_vars"])
    gmm = api.AmDiagGmm(gconsts, am["means_invvars"], am["inv_vars"], am["pdf_offsets"])
    adapted = dict(read_table(d / "adapted.ark", "matrix"))
    raw = read_table(d / "lat.tmp.ark", "lattice")
    clats = read_table(d / "lat.tmp.ark", "compact_lattice_converted")
    assert [k for k, _ in clats] == KEYS
    ls = tool("lattice-scale")
    scaled = [ls.scale_compact_lattice(np.array([[1.0, 0.0], [0.0, 0.0]]), c) for _, c in clats]
    rows = np.concatenate([[0], np.cumsum([len(adapted[k]) for k in KEYS])]).astype(np.int64)
    x = torch.from_numpy(np.ascontiguousarray(np.concatenate([adapted[k] for k in KEYS], 0), dtype=F)).cuda()
    res = api.gmm_rescore_compact_lattices(gmm, x, rows, scaled, tm["tid2pdf"])
    return dict(tm=tm, gmm=gmm, adapted=adapted, raw=raw, clats=clats, res=res, rows=rows, x=x)


def test_stage_4_the_rescored_table_equals_the_library_call_byte_for_byte(files, in_process, api):
    cli = pkg("kaldi_cli")
    d = files["dir"]
    assert all(r["status"] == api.RESCORE_OK for r in in_process["res"])
    w = cli.TableWriter("ark:" + str(d / "expected_resc.ark"), "compact_lattice")
    for k, r in zip(KEYS, in_process["res"]):
        w.write(k, r["clat"])
    w.close()
    assert (d / "resc.ark").read_bytes() == (d / "expected_resc.ark").read_bytes() and (d / "resc.ark").stat().st_size > 5000
    # the input really was a state-level table, and the conversion joined chains
    for (_, L), (_, c) in zip(in_process["raw"], in_process["clats"]):
        assert int(c["n_states"]) <= int(L["num_states"]) and len(c["arc_src"]) <= len(L["arc_src"])
        R.same_clat(c, R.convert_lattice(L))
    assert sum(int(L["num_states"]) - int(c["n_states"]) for (_, L), (_, c) in zip(in_process["raw"], in_process["clats"])) > 0
    # every acoustic cost is the sum of its string's scores alone (the old scores were scaled by 0.0): against the
    # restatement on the device's own matrix
    ll = in_process["gmm"].pdf_log_likelihoods(in_process["x"], log_sum_exp_prune=-1.0).cpu().numpy()
    rows = in_process["rows"]
    ls = tool("lattice-scale")
    for i, ((_, c), r) in enumerate(zip(in_process["clats"], in_process["res"])):
        status, want = R.rescore(ls.scale_compact_lattice(np.array([[1.0, 0.0], [0.0, 0.0]]), c), ll[rows[i]:rows[i + 1]], in_process["tm"]["tid2pdf"])
        assert status == R.OK
        R.same_clat(r["clat"], want, i)


def test_stage_4_the_determinized_table_equals_the_library_call(files, in_process, api):
    kio = pkg("kaldi_io")
    d = files["dir"]
    got = read_table(d / "lat.ark", "compact_lattice")
    assert [k for k, _ in got] == KEYS
    s = float(F(0.083333))
    for (_, g), r in zip(got, in_process["res"]):
        L = kio.compact_lattice_to_lattice(r["clat"])
        assert np.all(L["state_final_acoustic"][np.isfinite(L["state_final_graph"])] == 0)
        L["arc_a"] = (s * np.asarray(L["arc_a"], np.float64)).astype(F)
        L["state_final"] = np.asarray(L["state_final_graph"], F)
        det = api.determinize_lattice_pruned(L, float(F(6.0)), phone_determinize=False, word_determinize=True)
        det["arc_a"] = ((1.0 / s) * np.asarray(det["arc_a"], np.float64)).astype(F)
        with np.errstate(invalid="ignore"):
            det["final_a"] = np.where(det["final_g"] == np.inf, F(np.inf), ((1.0 / s) * np.asarray(det["final_a"], np.float64)).astype(F)).astype(F)
        R.same_clat(g, dict(det, start=0))
        assert g["n_states"] > 1
    err = files["pipe_err"]
    frames = sum(b - a for a, b in SPAN.values())
    assert "LOG (gmm-rescore-lattice:main()) Done 3 lattices with errors on 0, #frames is %d" % frames in err
    assert ("LOG (lattice-determinize-pruned:main()) Done 3 lattices, determinization finished earlier than specified by the beam on 0 of these."
            in err)
    assert "LOG (transform-feats:main()) Applied transform to 3 utterances; 0 had errors." in err


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_old_acoustic_scale_adds_the_scaled_old_costs(files, in_process, scale, monkeypatch):
    """new = the fold of the scores from scale * old; the default run's cost is the fold from 0 (the old score times 0.0).
    Both differ from the exact sums by the roundings of their adds alone - an item of len transition-ids has len adds in
    either fold, each within 1/2 ulp32 of a partial sum - and scale * old + default is one more add, so
    |new - (scale * old + default)| <= len * ulp32(M), M the largest magnitude among scale * old and the partial sums of
    the two folds (taken from the device's own matrix in float64, plus the bound itself)."""
    monkeypatch.chdir(files["dir"])
    out = "resc_%g.ark" % scale
    assert tool("gmm-rescore-lattice").main(["--old-acoustic-scale=%g" % scale, "final.mdl", "ark:lat.tmp.ark", "ark:adapted.ark", "ark:" + out]) == 0
    got = read_table(out, "compact_lattice")
    ll = in_process["gmm"].pdf_log_likelihoods(in_process["x"], log_sum_exp_prune=-1.0).cpu().numpy().astype(np.float64)
    t2p, rows = in_process["tm"]["tid2pdf"], in_process["rows"]
    worst = 0.0
    for i, ((_, g), (_, c), r) in enumerate(zip(got, in_process["clats"], in_process["res"])):
        dflt = r["clat"]
        assert np.array_equal(g["arc_src"], dflt["arc_src"]) and np.array_equal(g["arc_dst"], dflt["arc_dst"])
        assert g["arc_g"].tobytes() == dflt["arc_g"].tobytes()
        old = (scale * np.asarray(c["arc_a"], np.float64)).astype(F)
        times = R.compact_lattice_state_times(c)[1]
        for j in range(len(g["arc_a"])):
            n = len(c["arc_string"][j])
            want = float(old[j]) + float(dflt["arc_a"][j])
            t0 = rows[i] + times[int(c["arc_src"][j])]
            part = np.cumsum([-ll[t0 + k, t2p[int(x)]] for k, x in enumerate(c["arc_string"][j])]) if n else np.zeros(1)
            M = max(abs(float(old[j])), float(np.abs(part).max()), float(np.abs(part + float(old[j])).max()))
            M += n * float(np.spacing(F(M)))
            bound = n * float(np.spacing(F(M)))
            err = abs(float(g["arc_a"][j]) - want)
            worst = max(worst, err / bound if bound else err)
            assert err <= bound, (j, n, err, bound)
        assert np.any(old != 0)
    print("scale", scale, "worst error / bound", worst)


def test_missing_feature_key_warning_and_exit_status(files, in_process, monkeypatch, capfd):
    cli = pkg("kaldi_cli")
    monkeypatch.chdir(files["dir"])
    w = cli.TableWriter("ark:adapted_two.ark", "matrix")
    for k in ("utt0", "utt2"):
        w.write(k, in_process["adapted"][k])
    w.close()
    w = cli.TableWriter("ark:adapted_other.ark", "matrix")
    w.write("someone_else", in_process["adapted"]["utt0"])
    w.close()
    capfd.readouterr()
    assert tool("gmm-rescore-lattice").main(["final.mdl", "ark:lat.tmp.ark", "ark:adapted_two.ark", "ark:resc_two.ark"]) == 0
    err = capfd.readouterr().err
    assert "WARNING (gmm-rescore-lattice:main()) No feature found for utterance utt1. Skipping" in err
    frames = sum(SPAN[k][1] - SPAN[k][0] for k in ("utt0", "utt2"))
    assert "LOG (gmm-rescore-lattice:main()) Done 2 lattices with errors on 1, #frames is %d" % frames in err
    assert [k for k, _ in read_table("resc_two.ark", "compact_lattice")] == ["utt0", "utt2"]
    assert tool("gmm-rescore-lattice").main(["final.mdl", "ark:lat.tmp.ark", "ark:adapted_other.ark", "ark:resc_none.ark"]) == 1
    err = capfd.readouterr().err
    assert err.count("No feature found for utterance") == 3
    assert "LOG (gmm-rescore-lattice:main()) Done 0 lattices with errors on 3, #frames is 0" in err


def test_short_features_and_wrong_dimension(files, in_process, monkeypatch, capfd):
    cli = pkg("kaldi_cli")
    monkeypatch.chdir(files["dir"])
    utt_len = in_process["res"][1]["utt_len"]
    w = cli.TableWriter("ark:adapted_short.ark", "matrix")
    for k in KEYS:
        w.write(k, in_process["adapted"][k][:utt_len - 1] if k == "utt1" else in_process["adapted"][k])
    w.close()
    capfd.readouterr()
    assert tool("gmm-rescore-lattice").main(["--batch-frames=50", "final.mdl", "ark:lat.tmp.ark", "ark:adapted_short.ark", "ark:resc_short.ark"]) == 0
    err = capfd.readouterr().err
    assert ("WARNING (gmm-rescore-lattice:RescoreCompactLatticeInternal()) Features are too short for lattice: utt-len is %d, %d is last frame"
            % (utt_len, utt_len - 2)) in err
    assert "LOG (gmm-rescore-lattice:main()) Done 2 lattices with errors on 1" in err
    got = dict(read_table("resc_short.ark", "compact_lattice"))
    assert sorted(got) == ["utt0", "utt2"]                            # (three batches here: utt0 | utt1 | utt2)
    assert np.allclose(got["utt2"]["arc_a"], in_process["res"][2]["clat"]["arc_a"], rtol=1e-5, atol=1e-4)
    w = cli.TableWriter("ark:adapted_dim.ark", "matrix")
    w.write("utt0", in_process["adapted"]["utt0"][:, :12])
    w.close()
    assert tool("gmm-rescore-lattice").main(["final.mdl", "ark:lat.tmp.ark", "ark:adapted_dim.ark", "ark:resc_dim.ark"]) == 255
    assert "Dim mismatch: data dim = 12 vs. model dim = 13" in capfd.readouterr().err
