"""GPU: the fMLLR programs end to end on files (tools/fmllr_tools.py), through the bin/ shims as a recipe's pipe and in
process: the written float transforms against tests/fmllr_restatement.py on the same posteriors, with the tolerance the
restatement itself measures for them (fmllr_cases.e2e_reference: 4 x its own perturbed runs' difference, at least 1 ulp)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import fmllr_cases as C
import fmllr_restatement as R
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))


def tool(name):
    return importlib.import_module(name.replace("-", "_"))


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """final.mdl, feats.ark, ali.ark, spk2utt, utt2spk of the end-to-end case in one directory, and the restatement on the
    posteriors the pipe makes of them: ali-to-post | weight-silence-post 0.0 1 (phone 1 = transition-ids 1, 2 = pdf 0)."""
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    d = tmp_path_factory.mktemp("fmllr")
    am, feats, utt, spk, posts, tid2pdf = C.e2e_case(oracle)
    C.e2e_model_files(kio, am, str(d / "final.mdl"))
    ali = C.e2e_alignment(posts)
    keys = ["utt%d" % u for u in range(len(utt) - 1)]
    fw = cli.TableWriter("ark:" + str(d / "feats.ark"), "matrix")
    aw = cli.TableWriter("ark:" + str(d / "ali.ark"), "int32_vector")
    for u, k in enumerate(keys):
        fw.write(k, feats[utt[u]:utt[u + 1]])
        if k != "utt5":                                   # one utterance of speaker C has no alignment
            aw.write(k, np.asarray(ali[utt[u]:utt[u + 1]], np.int32))
    fw.close()
    aw.close()
    with open(d / "spk2utt", "w") as f, open(d / "utt2spk", "w") as g:
        for s, name in enumerate(C.E2E_SPK_NAMES):
            f.write(name + " " + " ".join(keys[spk[s]:spk[s + 1]]) + "\n")
            for k in keys[spk[s]:spk[s + 1]]:
                g.write("%s %s\n" % (k, name))
    tid2phone = np.array([0] + [(t - 1) // 2 + 1 for t in range(1, 13)], np.int32)
    tool_posts = R.weight_silence_post(tid2phone, [1], 0.0, [[(t, 1.0)] for t in ali])
    for t in range(int(utt[5]), int(utt[6])):
        tool_posts[t] = []                                # utt5: skipped by the estimator
    ref = C.e2e_reference(oracle, posts=tool_posts, types=["full", "diag"])
    return dict(dir=d, keys=keys, ref=ref, feats=feats, utt=utt, spk=spk, tool_posts=tool_posts, am=am, oracle=oracle)


def read_transforms(path):
    return dict(pkg("kaldi_io").read_ark(str(path)))


def check_transforms(got, files, ty):
    w_ref, impr_ref, count_ref = files["ref"]["ref"][ty]
    tol = C.transform_tolerance(w_ref, ty, measured=files["ref"]["diff"][ty])
    assert sorted(got) == sorted(C.E2E_SPK_NAMES)
    for s, name in enumerate(C.E2E_SPK_NAMES):
        err = np.abs(got[name].astype(np.float64) - w_ref[s])
        print(ty, name, "max err", err.max(), "tolerance", tol[s].min())
        assert got[name].shape == (13, 14) and (err <= tol[s]).all(), name
    assert np.array_equal(got["spkD"], np.eye(13, 14, dtype=np.float32))


def test_recipe_pipe_through_the_shims(files):
    """ali-to-post | weight-silence-post | gmm-est-fmllr --spk2utt with only bin/ in front of PATH, then transform-feats
    --utt2spk on the result, as steps/align_fmllr.sh and steps/decode_fmllr.sh write them."""
    d = files["dir"]
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    cmd = ("set -o pipefail; ali-to-post ark:ali.ark ark:- | weight-silence-post 0.0 1 final.mdl ark:- ark:- | "
           "gmm-est-fmllr --fmllr-update-type=full --fmllr-min-count=%g --spk2utt=ark:spk2utt final.mdl ark:feats.ark ark,s,cs:- ark:trans.ark"
           % C.E2E_MIN_COUNT)
    p = subprocess.run(["bash", "-c", cmd], cwd=d, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    err = p.stderr
    check_transforms(read_transforms(d / "trans.ark"), files, "full")
    assert "WARNING (gmm-est-fmllr:main()) Did not find posteriors for utterance utt5" in err
    assert "WARNING (gmm-est-fmllr:Update()) Not updating fMLLR since below min-count: count is" in err
    assert "LOG (gmm-est-fmllr:main()) Done 7 files, 1 with no posts, 0 with other errors." in err
    _, impr, count = files["ref"]["ref"]["full"]
    assert ("LOG (gmm-est-fmllr:main()) For speaker spkA, auxf-impr from fMLLR is %g, over %g frames." %
            (np.float32(impr[0]) / np.float32(count[0]), count[0]))[:70] in err
    assert "LOG (ali-to-post:main()) Converted 7 alignments." in err and "LOG (weight-silence-post:main()) Done 7 posteriors." in err
    p = subprocess.run(["bash", "-c", "transform-feats --utt2spk=ark:utt2spk ark:trans.ark ark:feats.ark ark:adapted.ark"], cwd=d, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "LOG (transform-feats:main()) Applied transform to 8 utterances; 0 had errors." in p.stderr
    assert "LOG (transform-feats:main()) Overall average logdet is " in p.stderr and " over 1460 frames." in p.stderr
    out = read_transforms(d / "adapted.ark")
    w_ref = files["ref"]["ref"]["full"][0]
    utt, spk = files["utt"], files["spk"]
    for s in range(4):
        for u in range(spk[s], spk[s + 1]):
            want = R.transform_feats(w_ref[s], files["feats"][utt[u]:utt[u + 1]])
            assert np.abs(out[files["keys"][u]] - want).max() < 1e-4


def test_tools_in_process(files, monkeypatch, capfd):
    """The gpost route (gmm-post-to-gpost | gmm-est-fmllr-gpost) gives the bits of the post route; --fmllr-update-type=diag;
    per utterance; compose-transforms then transform-feats; a transform of the wrong dimension."""
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    monkeypatch.chdir(files["dir"])
    w = cli.TableWriter("ark:post.ark", "posterior")
    utt = files["utt"]
    for u, k in enumerate(files["keys"]):
        if k != "utt5":
            w.write(k, files["tool_posts"][utt[u]:utt[u + 1]])
    w.close()
    mc = "--fmllr-min-count=%g" % C.E2E_MIN_COUNT
    assert tool("gmm-est-fmllr").main([mc, "--spk2utt=ark:spk2utt", "final.mdl", "ark:feats.ark", "ark:post.ark", "ark:t_post.ark"]) == 0
    assert tool("gmm-post-to-gpost").main(["final.mdl", "ark:feats.ark", "ark:post.ark", "ark:gpost.ark"]) == 0
    err = capfd.readouterr().err
    assert "LOG (gmm-post-to-gpost:main()) Done 7 files, 1 with no posteriors, 0 with other errors." in err
    assert "LOG (gmm-post-to-gpost:main()) Overall avg like per frame (Gaussian only) = " in err
    assert tool("gmm-est-fmllr-gpost").main([mc, "--spk2utt=ark:spk2utt", "final.mdl", "ark:feats.ark", "ark:gpost.ark", "ark:t_gpost.ark"]) == 0
    err = capfd.readouterr().err
    assert "LOG (gmm-est-fmllr-gpost:main()) Done 7 files, 1 with no gposts, 0 with other errors." in err
    a, b = read_transforms("t_post.ark"), read_transforms("t_gpost.ark")
    check_transforms(a, files, "full")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # diag
    assert tool("gmm-est-fmllr").main([mc, "--fmllr-update-type=diag", "--spk2utt=ark:spk2utt", "final.mdl", "ark:feats.ark", "ark:post.ark",
                                       "ark:t_diag.ark"]) == 0
    check_transforms(read_transforms("t_diag.ark"), files, "diag")
    # per utterance: one transform per utterance that has posteriors
    capfd.readouterr()
    assert tool("gmm-est-fmllr").main([mc, "final.mdl", "ark:feats.ark", "ark:post.ark", "ark:t_utt.ark"]) == 0
    err = capfd.readouterr().err
    assert "WARNING (gmm-est-fmllr:main()) Did not find posts for utterance utt5" in err
    per = read_transforms("t_utt.ark")
    assert sorted(per) == sorted(k for k in files["keys"] if k != "utt5")
    assert np.array_equal(per["utt0"], a["spkA"])          # speaker A is one utterance: the same statistics, the same bits
    assert np.array_equal(per["utt7"], np.eye(13, 14, dtype=np.float32))
    # compose with a second-pass transform, apply; and a transform that does not fit
    assert tool("compose-transforms").main(["--b-is-affine=true", "ark:t_diag.ark", "ark:t_post.ark", "ark:t_comp.ark"]) == 0
    assert tool("transform-feats").main(["--utt2spk=ark:utt2spk", "ark:t_comp.ark", "ark:feats.ark", "ark:adapted2.ark"]) == 0
    out = read_transforms("adapted2.ark")
    comp = R.compose_transforms(read_transforms("t_diag.ark")["spkB"], a["spkB"], True)
    assert np.abs(out["utt2"] - R.transform_feats(comp, files["feats"][utt[2]:utt[3]])).max() < 1e-4
    capfd.readouterr()
    assert tool("transform-feats").main(["ark:t_utt.ark", "ark:feats.ark", "ark:adapted3.ark"]) == 0
    err = capfd.readouterr().err
    assert "WARNING (transform-feats:main()) No fMLLR transform available for utterance utt5, producing no output for this utterance" in err
    assert "LOG (transform-feats:main()) Applied transform to 7 utterances; 1 had errors." in err


def shim_env():
    return dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)


def shell(files, cmd):
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=files["dir"], env=shim_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stderr


POSTS = "ali-to-post ark:ali.ark ark:- | weight-silence-post 0.0 1 final.mdl ark:- ark:- | "


def ensure_trans(files, monkeypatch):
    """trans0.ark: the full speaker transforms of the post route, in process (once per module)."""
    monkeypatch.chdir(files["dir"])
    if not os.path.exists("trans0.ark"):
        cli = pkg("kaldi_cli")
        w = cli.TableWriter("ark:post0.ark", "posterior")
        for u, k in enumerate(files["keys"]):
            if k != "utt5":
                w.write(k, files["tool_posts"][files["utt"][u]:files["utt"][u + 1]])
        w.close()
        assert tool("gmm-est-fmllr").main(["--fmllr-min-count=%g" % C.E2E_MIN_COUNT, "--spk2utt=ark:spk2utt", "final.mdl", "ark:feats.ark",
                                           "ark:post0.ark", "ark:trans0.ark"]) == 0
    return read_transforms("trans0.ark")


@pytest.mark.parametrize("update_type,per_utt", [("offset", True), ("none", False), ("full", True)])
def test_shims_update_types_and_per_utterance(files, update_type, per_utt):
    """The estimation pipe through the shims without --spk2utt (one transform per utterance that has posteriors) and with
    the update types the other tests leave out; the reference is the restatement on the pipe's own posteriors."""
    ref = C.e2e_reference(files["oracle"], per_utt=per_utt, posts=files["tool_posts"], types=[update_type])
    w_ref, impr_ref, count_ref = ref["ref"][update_type]
    out = "t_%s_%d.ark" % (update_type, per_utt)
    err = shell(files, POSTS + "gmm-est-fmllr --fmllr-update-type=%s --fmllr-min-count=%g %s final.mdl ark:feats.ark ark,s,cs:- ark:%s"
                % (update_type, C.E2E_MIN_COUNT, "" if per_utt else "--spk2utt=ark:spk2utt", out))
    got = read_transforms(files["dir"] / out)
    tol = C.transform_tolerance(w_ref, update_type, measured=ref["diff"][update_type])
    names = files["keys"] if per_utt else C.E2E_SPK_NAMES
    assert sorted(got) == sorted(k for k in names if k != "utt5")
    for s, name in enumerate(names):
        if name == "utt5":        # no alignment: no posteriors, no transform (the restatement's speaker there has no entries)
            assert "Did not find posts for utterance utt5" in err
            continue
        e = np.abs(got[name].astype(np.float64) - w_ref[s])
        print(update_type, name, "max err", e.max(), "tolerance", tol[s].min(), "count", count_ref[s])
        assert (e <= tol[s]).all(), name
        if not count_ref[s] > C.E2E_MIN_COUNT:
            assert np.array_equal(got[name], np.eye(13, 14, dtype=np.float32))
    if update_type == "none":
        assert all(np.array_equal(m, np.eye(13, 14, dtype=np.float32)) for m in got.values())
    if per_utt:
        assert (count_ref > C.E2E_MIN_COUNT).sum() >= 3 and (count_ref < C.E2E_MIN_COUNT).sum() >= 3
        assert "LOG (gmm-est-fmllr:main()) For utterance utt0, auxf-impr from fMLLR is" in err
    assert "LOG (gmm-est-fmllr:main()) Done 7 files, 1 with no posts, 0 with other errors." in err


def test_shims_gpost_route_and_compose(files, monkeypatch):
    """ali-to-post | weight-silence-post | gmm-post-to-gpost | gmm-est-fmllr-gpost --spk2utt, all four as shims in one pipe: the
    bits of the post route; then compose-transforms as a shim."""
    a = ensure_trans(files, monkeypatch)
    err = shell(files, POSTS + "gmm-post-to-gpost final.mdl ark:feats.ark ark,s,cs:- ark:- | gmm-est-fmllr-gpost --fmllr-min-count=%g "
                "--spk2utt=ark:spk2utt final.mdl ark:feats.ark ark,s,cs:- ark:t_gpost_shim.ark" % C.E2E_MIN_COUNT)
    assert "LOG (gmm-post-to-gpost:main()) Done converting post to gpost" in err
    assert "LOG (gmm-est-fmllr-gpost:main()) Done 7 files, 1 with no gposts, 0 with other errors." in err
    b = read_transforms(files["dir"] / "t_gpost_shim.ark")
    check_transforms(b, files, "full")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    shell(files, "compose-transforms --b-is-affine=true ark:t_gpost_shim.ark ark:trans0.ark ark:comp_shim.ark")
    c = read_transforms(files["dir"] / "comp_shim.ark")
    for k in a:
        assert c[k].shape == (13, 14) and np.abs(c[k] - R.compose_transforms(b[k], a[k], True)).max() < 1e-4


def test_transform_feats_as_a_stage_of_the_decoder_s_feature_pipe(files, monkeypatch):
    """The recipe's form: gmm-latgen-faster reads "ark,s,cs:... | transform-feats --utt2spk=... ark:trans ark:- ark:- |" - standard
    input and output both tables, the shim started by the decoder's own pipe - with only bin/ in front of PATH.  The lattices
    and words equal, byte for byte, those of the file route (transform-feats to an archive, then the decoder on it), and the
    adapted features of the pipe equal the file route's."""
    kio, workloads = pkg("kaldi_io"), pkg("workloads")
    ensure_trans(files, monkeypatch)
    rng = np.random.default_rng(41)
    g = workloads.make_hclg_like(rng, 300, 6, final_frac=0.2)
    g["tid2pdf"] = np.concatenate([[-1], np.repeat(np.arange(6), 2)]).astype(np.int32)
    with open("HCLG.fst", "wb") as f:
        kio.write_fst(f, g)
    opts = "--beam=10 --max-active=200 --lattice-beam=6 --acoustic-scale=0.1 --allow-partial=true --determinize-lattice=false"
    tf = "transform-feats --utt2spk=ark:utt2spk ark:trans0.ark"
    err = shell(files, "gmm-latgen-faster %s final.mdl HCLG.fst 'ark,s,cs:cat feats.ark | %s ark:- ark:- |' ark:lat_pipe.ark ark,t:words_pipe.txt"
                % (opts, tf))
    assert "LOG (transform-feats:main()) Applied transform to 8 utterances; 0 had errors." in err
    shell(files, "%s ark:feats.ark ark:adapted_file.ark && gmm-latgen-faster %s final.mdl HCLG.fst ark:adapted_file.ark ark:lat_file.ark "
          "ark,t:words_file.txt && %s ark:- ark:- < feats.ark > adapted_pipe.ark" % (tf, opts, tf))
    d = files["dir"]
    assert (d / "lat_pipe.ark").read_bytes() == (d / "lat_file.ark").read_bytes() and (d / "lat_pipe.ark").stat().st_size > 10000
    words = (d / "words_pipe.txt").read_text()
    assert words == (d / "words_file.txt").read_text() and len(words.splitlines()) == 8 and len(words.split()) > 8 + 20
    assert (d / "adapted_pipe.ark").read_bytes() == (d / "adapted_file.ark").read_bytes()
    # the features behind the pipe are the adapted ones: speaker A's first utterance against the restatement
    got = read_transforms(d / "adapted_pipe.ark")["utt0"]
    want = R.transform_feats(read_transforms(d / "trans0.ark")["spkA"], files["feats"][:files["utt"][1]])
    assert np.abs(got - want).max() < 1e-4
