"""GPU: gmm-acc-mllt end to end on files (tools/gmm_acc_mllt.py) through the bin/ shim, with PATH changed only, as
steps/train_lda_mllt.sh runs it: the written .macc, read back by kaldi_io.read_mllt_accs, against tests/mllt_restatement.py on
the same job.  The restatement runs in a child process, so that it and the tool both start from the generator of a process
that never seeded.

A flipped draw would swamp any bound, so the comparison stands under a CONDITION, asserted on the restatement's own values
(mllt_cases.margins_hold): no draw lies within 4 float ulps of the |p| / rand_prune it is compared with, and no |p| within 4
float ulps of the threshold.  Then the tool takes the restatement's branch at every posterior, and
  beta  is within the posteriors' bound (fmllr_cases.post_bound) summed over the survivors that are kept as themselves,
        plus both sides' summation bound;
  G     is within the summation bound plus the posteriors' bound carried through the sums (mllt_cases.carried_allowance).
At --rand-prune=4.0 every survivor is exactly +-4 and nothing is carried.

Three jobs, each run with --batch-frames=200 (two batches: 200 and 150 rows) and with the default (one batch):
  prune0   --rand-prune=0, the recipe's pipe: ali-to-post | weight-silence-post 0.0 1
  default  no option (0.25), fractional posteriors from an archive
  prune4   --rand-prune=4.0, fractional posteriors
test_batches_give_the_same_file_bits holds the two batchings to equal file bits: the tool accumulates utterance by utterance
(api.accumulate_mllt_stats with segments), positions the generator at every batch and lets beta run on, so nothing in the
file depends on --batch-frames."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import fmllr_cases as FC
import fmllr_restatement as R
import gmm_acc_cases as GC
import mllt_cases as C
import mllt_restatement as M
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu
JOBS = [("prune0", "--rand-prune=0", 0.0, True), ("default", "", 0.25, False), ("prune4", "--rand-prune=4.0", 4.0, False)]
PIPE = "ali-to-post ark:ali.ark ark:- | weight-silence-post 0.0 1 final.mdl ark:- ark:- | "


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """final.mdl, feats.ark, ali.ark, post.ark of a job of four utterances: utt1 (200 rows) and utt2 (150) are done, utt3's
    alignment and posterior are one frame short, uttX has features only.  Then the restatement of each job, each in a child
    process of its own."""
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    d = tmp_path_factory.mktemp("mllt")
    am, tid2pdf, utts = GC.e2e_utterances(oracle)
    FC.e2e_model_files(kio, am, str(d / "final.mdl"))
    utts = utts[1:4] + [("uttX", utts[4][1], utts[4][2], utts[4][3])]
    fw = cli.TableWriter("ark:" + str(d / "feats.ark"), "matrix")
    aw, pw = cli.TableWriter("ark:" + str(d / "ali.ark"), "int32_vector"), cli.TableWriter("ark:" + str(d / "post.ark"), "posterior")
    for key, mat, post, ali in utts:
        fw.write(key, mat)
        if key != "uttX":
            short = 1 if key == "utt3" else 0
            aw.write(key, np.asarray(ali[:len(ali) - short], np.int32))
            pw.write(key, post[:len(post) - short])
    for w in (fw, aw, pw):
        w.close()
    ow = cli.TableWriter("ark:" + str(d / "other.ark"), "posterior")
    ow.write("nobody", [[(1, 1.0)]])
    ow.close()
    done = utts[:2]
    tid2phone = np.array([-1] + [(t - 1) // 2 + 1 for t in range(1, len(tid2pdf))], np.int32)
    feats = np.concatenate([m for _, m, _, _ in done])
    ref = {}
    model = {k: am[k] for k in ("gconsts", "means_invvars", "inv_vars", "pdf_offsets")}
    for name, _, prune, pipe in JOBS:
        posts = [R.weight_silence_post(tid2phone, [1], 0.0, [[(int(t), 1.0)] for t in a]) if pipe else p for _, _, p, a in done]
        with open(d / (name + ".job"), "wb") as f:
            pickle.dump(dict(am=model, tid2pdf=tid2pdf, utts=[(m, p) for (_, m, _, _), p in zip(done, posts)]), f)
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mllt_restatement.py"), str(d / (name + ".job")), repr(prune),
                        str(d / (name + ".ref"))], check=True, timeout=300)
        with open(d / (name + ".ref"), "rb") as f:
            r = pickle.load(f)
        r["ent"] = R.entries_of(M.convert_posterior_to_pdfs(tid2pdf, [fr for p in posts for fr in p]), am["pdf_offsets"])
        assert len(r["acc"]["trace"]) == int(r["ent"]["goff"][-1])
        ref[name] = r
    return dict(dir=d, ref=ref, feats=feats, am=am)


def shell(files, cmd, status=0):
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=files["dir"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == status, p.stderr[-3000:]
    return p.stderr


@pytest.fixture(scope="module")
def runs(files):
    """Every command line once: the programs' standard error by job; the files are in files["dir"]."""
    out = {}
    for name, opt, _, pipe in JOBS:
        src = (PIPE, "ark,s,cs:-") if pipe else ("", "ark:post.ark")
        out[name] = shell(files, "%sgmm-acc-mllt %s final.mdl ark:feats.ark %s %s.macc" % (src[0], opt, src[1], name))
        out[name + "_b"] = shell(files, "%sgmm-acc-mllt --verbose=1 --batch-frames=200 %s final.mdl ark:feats.ark %s %s_b.macc" % (
            src[0], opt, src[1], name))
    return out


def read_acc(files, name):
    kio = pkg("kaldi_io")
    return kio.read_kaldi_object(str(files["dir"] / name), kio.read_mllt_accs)


def check_job(files, name, file_name):
    r = files["ref"][name]
    prune = dict((n, p) for n, _, p, _ in JOBS)[name]
    assert C.margins_hold(r["log"]), name                                # the condition, on the restatement's own values
    got, want = read_acc(files, file_name), r["acc"]
    am, ent = files["am"], r["ent"]
    post, pruned = want["trace"][:, 0], want["trace"][:, 1]
    o, w, p = C.items_of(am["pdf_offsets"], am["means_invvars"], am["inv_vars"], files["feats"], ent, pruned)
    kept = (pruned != 0) & (pruned.view(np.int32) == post.view(np.int32))          # survivors that are the posterior itself
    pb = np.where(kept, FC.post_bound(post, ent["goff"]), 0.0)[pruned != 0]
    if prune == 4.0:
        assert not pb.any() and set(np.abs(p).tolist()) == {4.0}
    if prune == 0.0:
        assert kept[post != 0].all() and r["draws"] == 0
    else:
        assert r["draws"] > 0
    n = len(p)
    assert got["dim"] == 13 == want["dim"] and got["G"].shape == (13, 91)
    # G: the restatement's own sums within the summation bound of the exact ones; the tool's within that plus what is carried
    print(name, file_name, "items", n, "draws", r["draws"], "restatement worst error / bound", C.check_bound(want["G"], o, w, 13, 3, name),
          "tool worst error / (bound + carried)",
          C.check_bound(got["G"], o, w, 13, 3, name + " tool", extra=C.carried_allowance(o, w, p, pb, 13, 3)))
    tol = float(pb.sum()) + 2 * (n + 2) * 2.0 ** -53 * float(np.abs(p.astype(np.float64)).sum())
    print(name, "beta", got["beta"], "restatement", want["beta"], "tolerance", tol)
    assert abs(got["beta"] - want["beta"]) <= tol
    if prune == 4.0:
        assert got["beta"] == want["beta"] == 4.0 * float((p > 0).sum()) - 4.0 * float((p < 0).sum())
    return got, r


@pytest.mark.parametrize("name", [j[0] for j in JOBS])
def test_file_against_the_restatement(files, runs, name):
    err = runs[name]
    got, r = check_job(files, name, name + ".macc")
    assert (files["dir"] / (name + ".macc")).read_bytes()[:13] == b"\0B<MlltAccs> "
    assert err.count("WARNING (gmm-acc-mllt:main()) Posterior vector has wrong size 89 vs. 90") == 1
    assert "LOG (gmm-acc-mllt:main()) Done 2 files, 1 with no posteriors, 1 with other errors." in err
    assert err.count("LOG (gmm-acc-mllt:main()) Average like for this file is ") == 2
    assert "LOG (gmm-acc-mllt:main()) Written accs." in err
    assert (" over %g frames." % r["tot_t"]) in err
    assert ("Overall avg like per frame (Gaussian only) = %g" % (r["tot_like"] / r["tot_t"]))[:48] in err
    for like, w in r["files"]:
        assert (" over %g frames." % w) in err


@pytest.mark.parametrize("name", [j[0] for j in JOBS])
def test_two_batches_against_the_restatement(files, runs, name):
    """--batch-frames=200 on utterances of 200 and 150 rows: two library passes; pruning goes on in utterance, frame, entry,
    Gaussian order across them, so the result is within the same bounds of the same restatement; beta, which runs on from
    batch to batch entry by entry, is the one-batch double."""
    assert [int(x) for x in re.findall(r"batch of (\d+) rows", runs[name + "_b"])] == [200, 150]
    got, _ = check_job(files, name, name + "_b.macc")
    one = read_acc(files, name + ".macc")
    assert got["beta"] == one["beta"]


@pytest.mark.parametrize("name", [j[0] for j in JOBS])
def test_batches_give_the_same_file_bits(files, runs, name):
    d = files["dir"]
    a, b = (d / (name + ".macc")).read_bytes(), (d / (name + "_b.macc")).read_bytes()
    ga, gb = read_acc(files, name + ".macc")["G"], read_acc(files, name + "_b.macc")["G"]
    diff = ga != gb
    print(name, "G doubles that differ between one batch and two:", int(diff.sum()), "of", ga.size, "largest relative difference",
          float((np.abs(ga - gb)[diff] / np.abs(ga[diff])).max()) if diff.any() else 0.0)
    assert len(a) == len(b) and a == b


def test_nothing_done_and_usage(files):
    err = shell(files, "gmm-acc-mllt final.mdl ark:feats.ark ark:other.ark empty.macc", status=1)
    assert "LOG (gmm-acc-mllt:main()) Done 0 files, 4 with no posteriors, 0 with other errors." in err
    got = read_acc(files, "empty.macc")
    assert got["beta"] == 0.0 and got["dim"] == 13 and got["G"].shape == (13, 91) and not got["G"].any()
    err = shell(files, "gmm-acc-mllt final.mdl ark:feats.ark ark:post.ark", status=1)
    assert "Accumulate MLLT (global STC) statistics" in err
    assert "Usage:  gmm-acc-mllt [options] <model-in> <feature-rspecifier> <posteriors-rspecifier> <stats-out>" in err
    assert "--rand-prune" in err and "--binary" in err and "--batch-frames" in err
    err = shell(files, "gmm-acc-mllt --binary=false --rand-prune=0 final.mdl ark:feats.ark ark:post.ark text.macc")
    text = (files["dir"] / "text.macc").read_bytes()
    assert text.startswith(b"<MlltAccs> \n") and text.endswith(b"]\n</MlltAccs> \n") and b" 13 <G> \n[\n" in text
    assert read_acc(files, "text.macc")["dim"] == 13
