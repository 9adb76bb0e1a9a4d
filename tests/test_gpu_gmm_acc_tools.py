"""GPU: the GMM accumulation programs end to end on files (tools/gmm_acc_tools.py) through the bin/ shims, with PATH changed
only, as a recipe runs them: the written .acc files, read back by kaldi_io.read_gmm_accs, against tests/gmm_acc_restatement.py
on the same job - transition accumulators equal as doubles, total_frames equal, total_like within the sum of the entries'
fmllr_cases.like_bound, the accumulators within the A1 bound carried through the sums (gmm_acc_cases.carried_bound) and a float
ulp; and, in a test of its own, their floats equal or adjacent (the count of unequal ones is printed).  A TEXT file cannot be
held to equal or adjacent floats: operator<< gives 7 significant digits, half a unit of the 7th being up to 5e-7 relative
against a float's 6e-8.  It is held to the binary file of the same run within that rounding (check_text), and the binary file
to the restatement.  Every program runs once, in a module fixture (runs); each test reads what it needs from it."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fmllr_cases as FC
import gmm_acc_cases as C
import gmm_acc_restatement as A
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """final.mdl, feats.ark, feats2.ark (9 dimensions), ali.ark(.gz), post.ark of a job of five utterances: utt0-2 are done,
    utt3's alignment and posterior are one frame short, uttX has features only."""
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    d = tmp_path_factory.mktemp("gmmacc")
    am, tid2pdf, utts = C.e2e_utterances(oracle)
    FC.e2e_model_files(kio, am, str(d / "final.mdl"))
    utts = utts[:4] + [("uttX", utts[4][1], utts[4][2], utts[4][3])]
    fw, f2 = cli.TableWriter("ark:" + str(d / "feats.ark"), "matrix"), cli.TableWriter("ark:" + str(d / "feats2.ark"), "matrix")
    aw, pw = cli.TableWriter("ark:" + str(d / "ali.ark"), "int32_vector"), cli.TableWriter("ark:" + str(d / "post.ark"), "posterior")
    for key, mat, post, ali in utts:
        fw.write(key, mat)
        if key != "uttX":
            f2.write(key, C.second_features(mat, 9, 3))
            short = 1 if key == "utt3" else 0
            aw.write(key, np.asarray(ali[:len(ali) - short], np.int32))
            pw.write(key, post[:len(post) - short])
    for w in (fw, f2, aw, pw):
        w.close()
    with open(d / "ali.ark", "rb") as f, gzip.open(d / "ali.ark.gz", "wb") as g:
        g.write(f.read())
    aw = cli.TableWriter("ark:" + str(d / "other.ark"), "int32_vector")
    aw.write("nobody", np.asarray([1, 2], np.int32))
    aw.close()
    done = utts[:3]
    ref = dict(ali=A.acc_stats_ali(am, tid2pdf, [(m, a) for _, m, _, a in done]),
               post=A.acc_stats(am, tid2pdf, [(m, p) for _, m, p, _ in done]),
               post_mw=A.acc_stats(am, tid2pdf, [(m, p) for _, m, p, _ in done], flags="mw"),
               two=A.acc_stats(am, tid2pdf, [(m, C.second_features(m, 9, 3), p) for _, m, p, _ in done], twofeats=True),
               two_ali=A.acc_stats(am, tid2pdf, [(m, C.second_features(m, 9, 3), [[(int(t), 1.0)] for t in a]) for _, m, _, a in done],
                                   twofeats=True))
    # the entries' posteriors and scores of each route over the stacked job, for the tolerances
    like = {}
    feats = np.concatenate([m for _, m, _, _ in done])
    for name, posts in (("ali", [[[(int(t), 1.0)] for t in a] for _, _, _, a in done]), ("post", [p for _, _, p, _ in done])):
        ent = A.R.entries_of(A.convert_posterior_to_pdfs(tid2pdf, [fr for p in posts for fr in p]), am["pdf_offsets"])
        post, lk = A.R.component_posteriors(am, feats, ent)
        like[name] = dict(like=lk, ent=ent, post=post)
    return dict(dir=d, ref=ref, like=like, feats=feats, feats2=C.second_features(feats, 9, 3), off=am["pdf_offsets"])


def shell(files, cmd, status=0):
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=files["dir"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == status, p.stderr[-3000:]
    return p.stderr


def read_acc(files, name):
    kio = pkg("kaldi_io")
    return kio.read_kaldi_object(str(files["dir"] / name), kio.read_gmm_accs)


# (label, file, the restatement's route, whose entries' scores and posteriors bound it, statistics from the second features)
ROUTES = [("gmm-acc-stats-ali", "ali.acc", "ali", "ali", False), ("three batches", "ali_b.acc", "ali", "ali", False),
          ("gmm-acc-stats", "post.acc", "post", "post", False), ("gmm-acc-stats mw", "post_mw.acc", "post_mw", "post", False),
          ("gmm-acc-stats-twofeats", "two.acc", "two", "post", True),
          ("ali-to-post | gmm-acc-stats-twofeats", "two_pipe.acc", "two_ali", "ali", True)]


@pytest.fixture(scope="module")
def runs(files):
    """Every accumulation command line once: the programs' standard error by group; the files are in files["dir"]."""
    return dict(
        ali=shell(files, "gmm-acc-stats-ali final.mdl ark:feats.ark ark:ali.ark ali.acc && "
                         "gmm-acc-stats-ali final.mdl ark:feats.ark 'ark,s,cs:gunzip -c ali.ark.gz |' ali_gz.acc"),
        batches=shell(files, "gmm-acc-stats-ali --verbose=1 --batch-frames=200 final.mdl ark:feats.ark ark:ali.ark ali_b.acc"),
        post=shell(files, "gmm-acc-stats final.mdl ark:feats.ark ark:post.ark post.acc && "
                          "gmm-acc-stats --update-flags=mw final.mdl ark:feats.ark ark:post.ark post_mw.acc && "
                          "gmm-acc-stats --update-flags=mw --binary=false final.mdl ark:feats.ark ark:post.ark post_mw.txt 2>/dev/null"),
        two=shell(files, "gmm-acc-stats-twofeats final.mdl ark:feats.ark ark:feats2.ark ark:post.ark two.acc && "
                         "ali-to-post ark:ali.ark ark:- | gmm-acc-stats-twofeats final.mdl ark:feats.ark ark:feats2.ark ark,s,cs:- two_pipe.acc"))


def check_route(files, label):
    """One route's file against the restatement: the accumulators within the A1 bound carried through the sums and a float
    ulp, the header, the transition accumulators as doubles, total_frames, total_like within the entries' like_bound."""
    _, name, route, like_of, two = next(r for r in ROUTES if r[0] == label)
    got = read_acc(files, name)
    want = files["ref"][route][0]
    le = files["like"][like_of]
    like, ent = le["like"], le["ent"]
    x2 = files["feats2"] if two else files["feats"]
    bound = C.carried_bound(files["off"], x2, ent, le["post"], want["flags"])
    for k in bound:                                        # the file holds floats: one rounding more
        if bound[k] is not None:
            bound[k] = bound[k] + np.spacing(np.abs(want[k]).astype(np.float32)).astype(np.float64)
    C.check_carried(got, want, bound, label)
    assert got["flags"] == want["flags"] and got["dim"] == want["dim"] and np.array_equal(got["pdf_offsets"], want["pdf_offsets"])
    assert np.array_equal(got["transition_accs"], want["transition_accs"]) and got["transition_accs"].dtype == np.float64
    assert got["total_frames"] == want["total_frames"]
    tol = float((FC.like_bound(like, ent["goff"]) * np.abs(ent["weight"].astype(np.float64))).sum())
    tol += float(np.abs(np.spacing((like * ent["weight"]).astype(np.float32))).sum())
    print(label, "total_like", got["total_like"], "reference", want["total_like"], "tolerance", tol)
    assert abs(got["total_like"] - want["total_like"]) <= tol
    return got


def test_acc_stats_ali(files, runs):
    """From an alignment archive and from the recipes' gunzip pipe; the missing key and the short alignment are warned of;
    the file carries the flags of Init(am_gmm, kGmmAll): 15."""
    err = runs["ali"]
    assert err.count("WARNING (gmm-acc-stats-ali:main()) No alignment for utterance uttX") == 2
    assert err.count("WARNING (gmm-acc-stats-ali:main()) Alignments has wrong size 89 vs. 90") == 2
    assert err.count("LOG (gmm-acc-stats-ali:main()) Done 3 files, 2 with errors.") == 2
    assert "LOG (gmm-acc-stats-ali:main()) Overall avg like per frame (Gaussian only) = " in err and " over 820 frames." in err
    assert "LOG (gmm-acc-stats-ali:main()) Written accs." in err
    d = files["dir"]
    data = (d / "ali.acc").read_bytes()
    assert data == (d / "ali_gz.acc").read_bytes() and data[:5] == b"\0BDV "
    assert data.count(b"<FLAGS> \xfe\x0f\x00<OCCUPANCY> ") == 6 and data.count(b"<FLAGS> ") == 6       # every pdf: kGmmAll
    got = check_route(files, "gmm-acc-stats-ali")
    assert got["flags"] == 15 and got["total_frames"] == 820.0
    acc, tot_like, tot_t = files["ref"]["ali"]
    assert ("Overall avg like per frame (Gaussian only) = %g" % (tot_like / tot_t))[:50] in err


def test_batches_and_sum(files, runs):
    """--batch-frames=200 on utterances of 470, 200 and 150 rows: three batches.  An utterance that would take a batch over
    the figure starts the next one, so 200 and 150 are apart; only the utterance longer than the figure is a batch above it,
    alone.  The result stays within the same bounds.  Then the two job files through gmm-sum-accs to standard output and from
    standard input, as the recipes' "gmm-sum-accs - $dir/$x.*.acc |"."""
    rows = [int(x) for x in re.findall(r"batch of (\d+) rows", runs["batches"])]
    assert rows == [470, 200, 150]
    check_route(files, "three batches")
    err = shell(files, "gmm-sum-accs - ali.acc ali_b.acc | gmm-sum-accs sum.acc - ali.acc")
    assert "LOG (gmm-sum-accs:main()) Summed 2 stats, total count 1640, avg like/frame " in err
    assert "LOG (gmm-sum-accs:main()) Summed 2 stats, total count 2460, avg like/frame " in err
    a, b, s = read_acc(files, "ali.acc"), read_acc(files, "ali_b.acc"), read_acc(files, "sum.acc")
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.array_equal(s[k], f32(f32(a[k] + b[k]) + a[k])), k                 # floats from disk, added in double, written as floats
    assert np.array_equal(s["transition_accs"], (a["transition_accs"] + b["transition_accs"]) + a["transition_accs"])
    assert s["total_frames"] == 2460.0 and s["total_like"] == (a["total_like"] + b["total_like"]) + a["total_like"]


def check_text(got, binary):
    """A text file against the binary file of the same run: every value through operator<< at 7 significant digits (half a
    unit of the 7th digit: 5e-7 relative) and back to a float (2^-24); whole numbers up to 10^7 are exact."""
    for k in ("occ", "mean_acc", "var_acc", "transition_accs"):
        assert (got[k] is None) == (binary[k] is None), k
        if binary[k] is not None:
            assert (np.abs(got[k] - binary[k]) <= (5e-7 + 2.0 ** -24) * np.abs(binary[k])).all(), k
    assert np.array_equal(got["transition_accs"], binary["transition_accs"]) and got["total_frames"] == binary["total_frames"]
    assert abs(got["total_like"] - binary["total_like"]) <= 5e-7 * abs(binary["total_like"])
    assert (got["flags"], got["dim"], got["pdf_offsets"].tolist()) == (binary["flags"], binary["dim"], binary["pdf_offsets"].tolist())


def test_acc_stats_update_flags(files, runs):
    """A posterior archive with two transition-ids of one pdf in a frame.  The default --update-flags=mvwt writes 15;
    --update-flags=mw leaves the variances out and writes 5; text mode."""
    err = runs["post"]
    assert err.count("WARNING (gmm-acc-stats:main()) Could not find posteriors for utterance uttX") == 2
    assert err.count("WARNING (gmm-acc-stats:main()) Posterior vector has wrong size 89 vs. 90") == 2
    assert err.count("LOG (gmm-acc-stats:main()) Done 3 files, 2 with errors.") == 2
    full = check_route(files, "gmm-acc-stats")
    assert full["flags"] == 15 and full["var_acc"].shape == (28, 13)
    assert (files["dir"] / "post.acc").read_bytes().count(b"<FLAGS> \xfe\x0f\x00") == 6
    got = check_route(files, "gmm-acc-stats mw")
    assert got["flags"] == 5 and got["var_acc"] is None and got["mean_acc"].shape == (28, 13)
    assert (files["dir"] / "post_mw.acc").read_bytes().count(b"<FLAGS> \xfe\x05\x00") == 6
    assert np.array_equal(got["occ"], full["occ"]) and np.array_equal(got["mean_acc"], full["mean_acc"])
    acc, tot_like, tot_t = files["ref"]["post_mw"]
    assert (" over %g frames." % tot_t) in err
    text = (files["dir"] / "post_mw.txt").read_bytes()
    assert text.startswith(b" [ 0 ") and text.count(b"<FLAGS> 5 <OCCUPANCY>") == 6
    check_text(read_acc(files, "post_mw.txt"), got)                       # the same run in text mode


def test_acc_stats_twofeats(files, runs):
    """Posteriors from the 13-dimensional features, statistics from the 9-dimensional ones; then the recipe's pipe from
    ali-to-post.  Init(am_gmm, new_dim, kGmmAll): 15."""
    err = runs["two"]
    assert err.count("WARNING (gmm-acc-stats-twofeats:main()) For utterance uttX, second features not present.") == 2
    assert err.count("WARNING (gmm-acc-stats-twofeats:main()) Posteriors has wrong size 89 vs. 90") == 2
    assert err.count("LOG (gmm-acc-stats-twofeats:main()) Done 3 files, 0 with no posteriors, 1 with no second features, 1 with other errors.") == 2
    assert err.count("LOG (gmm-acc-stats-twofeats:main()) Average like for this file is ") == 6
    got = check_route(files, "gmm-acc-stats-twofeats")
    assert got["dim"] == 9 and got["flags"] == 15 and got["var_acc"].shape == (28, 9)
    assert (files["dir"] / "two.acc").read_bytes().count(b"<FLAGS> \xfe\x0f\x00") == 6
    assert check_route(files, "ali-to-post | gmm-acc-stats-twofeats")["flags"] == 15


def test_empty_job_and_usage(files):
    err = shell(files, "gmm-acc-stats-ali final.mdl ark:feats.ark ark:other.ark empty.acc", status=1)
    assert err.count("WARNING (gmm-acc-stats-ali:main()) No alignment for utterance ") == 5
    assert "LOG (gmm-acc-stats-ali:main()) Done 0 files, 5 with errors." in err
    got = read_acc(files, "empty.acc")
    assert not got["occ"].any() and not got["transition_accs"].any() and got["total_frames"] == 0.0 and len(got["occ"]) == 28
    assert got["flags"] == 15
    err = shell(files, "gmm-acc-stats-ali final.mdl ark:feats.ark ark:ali.ark", status=1)
    assert "Usage:  gmm-acc-stats-ali [options] <model-in> <feature-rspecifier> <alignments-rspecifier> <stats-out>" in err
    err = shell(files, "gmm-acc-stats final.mdl ark:feats.ark", status=1)
    assert "--update-flags" in err and "Usage:  gmm-acc-stats [options]" in err


def test_written_floats_equal_or_adjacent(files, runs):
    """The binary files' floats against the restatement's as written, for every route: equal or adjacent floats, the count of
    unequal ones printed."""
    for label, name, route, _, _ in ROUTES:
        C.compare_written(read_acc(files, name), A.as_written(files["ref"][route][0]), label)
