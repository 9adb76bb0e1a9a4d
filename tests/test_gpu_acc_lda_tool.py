"""GPU: acc-lda end to end on files (tools/acc_lda.py) through the bin/ shim, with PATH changed only, as
steps/train_lda_mllt.sh runs it.  A 5-pdf transition model (followed in final.mdl by bytes nobody may read), D = 13, six
utterances:
  a  30 frames, done            b  0 frames with an empty posterior, done          c  60 frames, done
  d  45 frames, its posterior one frame short: a failure                           e  20 frames of 12 dimensions: a failure
  f  25 frames, no posterior: a failure
The written file equals kaldi_io.write_lda_accs of the in-process api.accumulate_lda_stats on the same input (seed 1, the
utterances as segments) byte for byte, at --rand-prune 0 and 4.0, in binary and in text, and whatever --batch-frames.
That accumulator is within the summation bound (tests/lda_cases.py) of the exact sums over the restatement's items
(tests/lda_restatement.py's loop after srand(1), the state of a process that never seeded), as is the restatement's own;
the counts agree bit for bit (weights that are multiples of 2^-10: every order is exact).
Fails without bin/acc-lda."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import lda_cases as C
import lda_restatement as L
import mllt_restatement as M
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu
NUM_PDFS, DIM = 5, 13


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    d = tmp_path_factory.mktemp("acclda")
    n = NUM_PDFS
    topo = dict(phones=list(range(1, n + 1)), phone2idx=[-1] + [0] * n, entries=[[(0, [(0, 0.5), (1, 0.5)]), (-1, [])]])
    log_probs = np.concatenate([[0.0], np.log(np.tile([0.75, 0.25], n))]).astype(np.float32)
    with open(d / "final.mdl", "wb") as f:
        f.write(b"\0B")
        kio.write_transition_model(f, topo, [(p + 1, 0, p) for p in range(n)], log_probs, True)
        f.write(b"<NotAnAmDiagGmm> only the transition model is read")
    tid2pdf = np.array([-1] + [p for p in range(n) for _ in range(2)], np.int32)      # transition-ids 2 p + 1, 2 p + 2 -> pdf p
    rng = np.random.default_rng(7)
    utts = {}
    for key, T, dim in (("a", 30, DIM), ("b", 0, DIM), ("c", 60, DIM), ("d", 45, DIM), ("e", 20, DIM - 1), ("f", 25, DIM)):
        mat = (rng.standard_normal((T, dim)) * 2 + 0.5).astype(np.float32)
        post = []
        for _ in range(T):
            k = int(rng.choice([0, 1, 1, 2, 3]))                                      # two transition-ids of one pdf are summed
            post.append([(int(t), float(w)) for t, w in zip(rng.choice(np.arange(1, 2 * n + 1), k, replace=False),
                                                           rng.choice([1.0, 0.5, 0.25, 0.125, -0.5], k))])
        utts[key] = (mat, post)
    fw, pw = cli.TableWriter("ark:" + str(d / "feats.ark"), "matrix"), cli.TableWriter("ark:" + str(d / "post.ark"), "posterior")
    for key, (mat, post) in utts.items():
        fw.write(key, mat)
        if key != "f":
            pw.write(key, post[:-1] if key == "d" else post)
    ow = cli.TableWriter("ark:" + str(d / "other.ark"), "posterior")
    ow.write("nobody", [[(1, 1.0)]])
    for w in (fw, pw, ow):
        w.close()
    return dict(dir=d, utts=utts, tid2pdf=tid2pdf)


def shell(files, cmd, status=0):
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable)
    p = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], cwd=files["dir"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == status, p.stderr[-3000:]
    return p.stderr


@pytest.fixture(scope="module")
def runs(files):
    """Every command line once: the programs' standard error by name; the files are in files["dir"]."""
    out = {}
    for name, opt in (("p0", ""), ("p4", "--rand-prune=4.0"), ("p0_text", "--binary=false"), ("p4_text", "--binary=false --rand-prune=4.0"),
                      ("p0_b", "--verbose=1 --batch-frames=50"), ("p4_b", "--verbose=1 --batch-frames=50 --rand-prune=4.0")):
        out[name] = shell(files, "acc-lda %s final.mdl ark:feats.ark ark:post.ark %s.acc" % (opt, name))
    return out


@pytest.fixture(scope="module")
def in_process(api, files):
    """api.accumulate_lda_stats on the utterances that are done (b has no rows), the utterances as segments, and the
    restatement of the whole job, per rand_prune."""
    done = [files["utts"][k] for k in ("a", "c")]
    feats = np.concatenate([m for m, _ in done])
    posts = [fr for _, p in done for fr in p]
    pdf_posts = api.convert_posterior_to_pdfs(files["tid2pdf"], posts)
    out = {}
    for prune in (0.0, 4.0):
        acc = api.accumulate_lda_stats(torch.from_numpy(feats).cuda(), pdf_posts, NUM_PDFS, rand_prune=prune, seed=1, segments=[0, 30, 90])
        M.srand(1)                                                           # the generator of a process that never seeded
        trace = []
        job = [(m, None if k == "f" else (p[:-1] if k == "d" else p)) for k, (m, p) in files["utts"].items()]
        ref, n_done, n_fail = L.acc_lda(NUM_PDFS, files["tid2pdf"], job, prune, trace=trace)
        out[prune] = dict(acc=acc, ref=ref, done=n_done, fail=n_fail, feats=feats, pdf_posts=pdf_posts,
                          pruned=np.asarray(trace, np.float32).reshape(-1, 2)[:, 1])
    return out


def file_bytes(acc, binary):
    f = io.BytesIO()
    pkg("kaldi_io").write_lda_accs(f, acc, binary)
    return (b"\0B" if binary else b"") + f.getvalue()


@pytest.mark.parametrize("name,prune,binary", [("p0", 0.0, True), ("p4", 4.0, True), ("p0_text", 0.0, False), ("p4_text", 4.0, False),
                                               ("p0_b", 0.0, True), ("p4_b", 4.0, True)])
def test_file_is_the_in_process_accumulator(files, runs, in_process, name, prune, binary):
    err = runs[name]
    data = (files["dir"] / (name + ".acc")).read_bytes()
    assert data == file_bytes(in_process[prune]["acc"], binary)
    assert data.startswith(b"\0B<LDAACCS> <VECSIZE> \x04\x0d\x00\x00\x00<NUMCLASSES> \x04\x05\x00\x00\x00" if binary
                           else b"<LDAACCS> <VECSIZE> 13 <NUMCLASSES> 5 <ZERO_ACCS>  [ ")
    assert err.count("WARNING (acc-lda:main()) No posteriors for utterance f") == 1
    assert err.count("WARNING (acc-lda:main()) Posterior vs. feats size mismatch 45 vs. 44") == 1
    assert err.count("WARNING (acc-lda:main()) Feature dimension mismatch 13 vs. 12") == 1
    assert "LOG (acc-lda:main()) Done 3 files, failed for 3" in err and "LOG (acc-lda:main()) Written statistics." in err
    assert (in_process[prune]["done"], in_process[prune]["fail"]) == (3, 3)
    if name.endswith("_b"):                                                  # a (30 rows), then c (60): two library passes
        assert [int(x) for x in re.findall(r"batch of (\d+) rows", err)] == [30, 60]
        assert data == (files["dir"] / (name[:-2] + ".acc")).read_bytes()


@pytest.mark.parametrize("prune", [0.0, 4.0])
def test_accumulator_against_the_restatement(in_process, prune):
    r = in_process[prune]
    ent = pkg("api").lda_entries(r["pdf_posts"])
    assert len(r["pruned"]) == len(ent["weight"])                            # the restatement met the same entries in the same order
    if prune == 0.0:
        assert np.array_equal(r["pruned"], ent["weight"])
    else:
        assert set(np.abs(r["pruned"]).tolist()) == {0.0, 4.0} and r["acc"]["draws"] == len(ent["weight"])
    ent["weight"] = r["pruned"]
    x, w, cls = C.items_of(r["feats"], ent)
    assert C.zero_is_exact(w) and np.array_equal(r["acc"]["zero"], r["ref"]["zero"])
    print("rand_prune", prune, "items", len(w), "of", len(r["pruned"]), "tool's accumulator worst error / bound",
          C.check_bound(r["acc"], x, w, cls, 3, "accumulate_lda_stats"), "restatement", C.check_bound(r["ref"], x, w, cls, 3, "restatement"))


def test_nothing_done_and_usage(files):
    err = shell(files, "acc-lda final.mdl ark:feats.ark ark:other.ark empty.acc", status=1)
    assert "LOG (acc-lda:main()) Done 0 files, failed for 6" in err and err.count("No posteriors for utterance") == 6
    kio = pkg("kaldi_io")
    data = (files["dir"] / "empty.acc").read_bytes()
    assert data == b"\0B" + L.write(L.empty(), True)                         # LdaEstimate::Init was never reached
    got = kio.read_kaldi_object(str(files["dir"] / "empty.acc"), kio.read_lda_accs)
    assert got["dim"] == 0 and got["num_classes"] == 0
    err = shell(files, "acc-lda final.mdl ark:feats.ark ark:post.ark", status=1)
    assert "Accumulate LDA statistics based on pdf-ids." in err
    assert "Usage:  acc-lda [options] <transition-gmm/model> <features-rspecifier> <posteriors-rspecifier> <lda-acc-out>" in err
    assert "--rand-prune" in err and "--binary" in err and "--batch-frames" in err
    # the recipe's pipe: sum-lda-accs over two job files reads what acc-lda wrote
    shell(files, "acc-lda final.mdl ark:feats.ark ark:post.ark j1.acc && sum-lda-accs sum.acc j1.acc j1.acc")
    one = kio.read_kaldi_object(str(files["dir"] / "j1.acc"), kio.read_lda_accs)
    two = kio.read_kaldi_object(str(files["dir"] / "sum.acc"), kio.read_lda_accs)
    assert np.allclose(two["second"], 2 * one["second"], rtol=1e-6) and np.allclose(two["zero"], 2 * one["zero"], rtol=1e-6)
