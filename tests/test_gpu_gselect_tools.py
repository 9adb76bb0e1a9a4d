"""GPU: gmm-gselect -> gmm-global-acc-stats --gselect -> gmm-global-sum-accs end to end on files (tools/gmm_gselect.py,
tools/gmm_global_acc_stats.py, tools/gmm_global_sum_accs.py), in process.  A DiagGmm of 9 Gaussians, D = 4, three utterances
of features: a (12 frames), b (7), c (5).  The second-pass gselect input has no entry for b and an entry of the wrong size
for c.  The gselect archive is byte-equal for two --batch-frames values and equals the restatement in library mode
(tests/gselect_restatement.py); --write-likes holds the double sums of the frames' floats; the .acc file read back is within
the bound tests/gmm_acc_cases.py derives; counts, warnings and exit statuses are the binaries'.  Fails without the tools."""
import importlib
import io
import os
import sys

import numpy as np
import pytest

import gmm_acc_cases as AC
import gselect_restatement as R
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
F32 = np.float32
G, D, N = 9, 4, 3
LENS = dict(a=12, b=7, c=5)


def tool(name):
    return importlib.import_module(name.replace("-", "_"))


@pytest.fixture(scope="module")
def files(tmp_path_factory, api):
    cli, kio = pkg("kaldi_cli"), pkg("kaldi_io")
    d = tmp_path_factory.mktemp("gselect_tools")
    rng = np.random.default_rng(5)
    weights = rng.dirichlet(np.full(G, 2.0)).astype(F32)
    iv = rng.uniform(0.5, 2.0, (G, D)).astype(F32)
    mi = (rng.standard_normal((G, D)) * iv).astype(F32)
    with open(d / "0.dubm", "wb") as f:
        f.write(b"\0B")
        kio.write_diag_gmm(f, weights, mi, iv, True)
    gconsts, _ = api.gmm_compute_gconsts(weights, mi, iv)
    utts = {k: rng.standard_normal((n, D)).astype(F32) for k, n in LENS.items()}
    w = cli.TableWriter("ark:" + str(d / "feats.ark"), "matrix")
    for k, m in utts.items():
        w.write(k, m)
    w.close()
    return dict(dir=d, utts=utts, model=dict(gconsts=gconsts, means_invvars=mi, inv_vars=iv))


def table_bytes(entries, kind):
    kio = pkg("kaldi_io")
    f = io.BytesIO()
    for k, v in entries:
        f.write(k.encode() + b" \0B")
        kio._write_object(f, True, kind, v)
    return f.getvalue()


def test_pipeline(files, monkeypatch, capfd):
    monkeypatch.chdir(files["dir"])
    kio = pkg("kaldi_io")
    m, utts = files["model"], files["utts"]
    want = {k: R.gaussian_selection(m, x, N) for k, x in utts.items()}
    # gmm-gselect: the archive for two --batch-frames values, the likes
    assert tool("gmm-gselect").main(["--n=%d" % N, "--write-likes=ark:likes.ark", "0.dubm", "ark:feats.ark", "ark:gselect.ark"]) == 0
    err = capfd.readouterr().err
    assert tool("gmm-gselect").main(["--n=%d" % N, "--batch-frames=8", "0.dubm", "ark:feats.ark", "ark:gselect.b.ark"]) == 0
    capfd.readouterr()
    got = (files["dir"] / "gselect.ark").read_bytes()
    assert got == (files["dir"] / "gselect.b.ark").read_bytes()
    assert got == table_bytes([(k, want[k][0]) for k in "abc"], "int32_vector_vector")
    likes = {k: sum(float(v) for v in want[k][1]) for k in "abc"}            # one part each: the frames in order, in double
    assert (files["dir"] / "likes.ark").read_bytes() == table_bytes([(k, likes[k]) for k in "abc"], "base_float")
    tot = likes["a"] + likes["b"] + likes["c"]
    assert "LOG (gmm-gselect:main()) For 0'th file, average UBM likelihood over 12 frames is %g" % (likes["a"] / 12) in err
    assert "LOG (gmm-gselect:main()) Done 3 files, 0 with errors, average UBM log-likelihood is %g over 24 frames." % (tot / 24) in err
    assert "WARNING" not in err
    # n above the number of Gaussians: the warning, the clamp
    assert tool("gmm-gselect").main(["--n=20", "0.dubm", "ark:feats.ark", "ark:all.ark"]) == 0
    err = capfd.readouterr().err
    assert ("WARNING (gmm-gselect:main()) You asked for 20 Gaussians but GMM only has 9, returning this many. Note: this means the "
            "Gaussian selection is pointless.") in err
    assert all(len(v) == G for _, u in kio.read_ark(str(files["dir"] / "all.ark"), "int32_vector_vector") for v in u)
    # a second pass limited to the first one's lists: b has no entry, c's has the wrong size
    with open("pre.ark", "wb") as f:
        f.write(table_bytes([("a", want["a"][0]), ("c", want["c"][0][:-1])], "int32_vector_vector"))
    assert tool("gmm-gselect").main(["--n=2", "--gselect=ark:pre.ark", "0.dubm", "ark:feats.ark", "ark,t:second.ark"]) == 0
    err = capfd.readouterr().err
    assert err.count("WARNING (gmm-gselect:main()) No gselect information for utterance b") == 1
    assert err.count("WARNING (gmm-gselect:main()) Input gselect for utterance c has wrong size 4 vs. 5") == 1
    assert "Done 1 files, 2 with errors" in err
    second = R.gaussian_selection(m, utts["a"], 2, want["a"][0])[0]
    assert (files["dir"] / "second.ark").read_bytes() == b"a " + b"".join(b"".join(b"%d " % g for g in v) + b"; " for v in second) + b"\n"
    with open("other.ark", "wb") as f:
        f.write(table_bytes([("nobody", [[1]])], "int32_vector_vector"))
    assert tool("gmm-gselect").main(["--gselect=ark:other.ark", "0.dubm", "ark:feats.ark", "ark:none.ark"]) == 1       # nothing done
    assert "Done 0 files, 3 with errors" in capfd.readouterr().err

    # gmm-global-acc-stats --gselect: the same missing entry and wrong size, per-frame weights
    wts = {k: np.random.default_rng(len(k) + n).choice([1.0, 0.5, 0.0], n).astype(F32) for k, n in LENS.items()}
    with open("weights.ark", "wb") as f:
        f.write(table_bytes([(k, wts[k]) for k in "abc"], "vector"))
    assert tool("gmm-global-acc-stats").main(["--gselect=ark:pre.ark", "--weights=ark:weights.ark", "0.dubm", "ark:feats.ark", "1.1.acc"]) == 0
    err = capfd.readouterr().err
    assert err.count("WARNING (gmm-global-acc-stats:main()) No gselect information for utterance b") == 1
    assert err.count("WARNING (gmm-global-acc-stats:main()) gselect information for utterance c has wrong size 4 vs. 5") == 1
    assert "LOG (gmm-global-acc-stats:main()) Done 1 files; 2 with errors." in err
    ra = R.global_acc_stats(m, utts["a"], want["a"][0], wts["a"], 7)
    assert ("LOG (gmm-global-acc-stats:main()) Overall likelihood per frame = %g over %g (weighted) frames."
            % (float(ra["file_like"]) / float(ra["file_weight"]), float(ra["file_weight"]))) in err
    assert "LOG (gmm-global-acc-stats:main()) Written accs to 1.1.acc" in err
    with open("1.1.acc", "rb") as f:
        assert f.read(2) == b"\0B"
        acc1 = kio.read_global_gmm_accs(f, True)
    assert acc1["flags"] == 7 and acc1["dim"] == D
    check_written(acc1, ra, utts["a"])
    # the whole first-pass archive, no weights, two batch sizes: the sums' grouping differs, both within the bound
    for name, extra in (("1.2.acc", []), ("1.3.acc", ["--batch-frames=8"])):
        assert tool("gmm-global-acc-stats").main(extra + ["--gselect=ark:gselect.ark", "0.dubm", "ark:feats.ark", name]) == 0
        assert "Done 3 files; 0 with errors." in capfd.readouterr().err
    x = np.concatenate([utts[k] for k in "abc"])
    rall = R.global_acc_stats(m, x, [v for k in "abc" for v in want[k][0]], None, 7)
    with open("1.2.acc", "rb") as f:
        f.read(2)
        acc2 = kio.read_global_gmm_accs(f, True)
    check_written(acc2, rall, x)
    # a list with a Gaussian twice: the utterance is an error, with a warning naming it; nothing done: status 1, file written
    dup = [np.asarray(v) for v in want["a"][0]]
    dup[3] = np.asarray([dup[3][0], dup[3][1], dup[3][0]], np.int32)
    with open("dup.ark", "wb") as f:
        f.write(table_bytes([("a", dup)], "int32_vector_vector"))
    assert tool("gmm-global-acc-stats").main(["--gselect=ark:dup.ark", "--update-flags=m", "0.dubm", "ark:feats.ark", "none.acc"]) == 1
    err = capfd.readouterr().err
    assert ("WARNING (gmm-global-acc-stats:main()) gselect information for utterance a cannot be used: frame 3 lists Gaussian %d twice"
            % dup[3][0]) in err
    assert "Done 0 files; 3 with errors." in err
    with open("none.acc", "rb") as f:
        f.read(2)
        none = kio.read_global_gmm_accs(f, True)
    assert none["flags"] == 5 and not none["occ"].any() and none["var_acc"] is None

    # gmm-global-sum-accs: the files' floats added in double in argument order; "-" is standard output
    assert tool("gmm-global-sum-accs").main(["sum.acc", "1.1.acc", "1.2.acc"]) == 0
    assert "LOG (gmm-global-sum-accs:main()) Written stats to sum.acc" in capfd.readouterr().err
    with open("sum.acc", "rb") as f:
        f.read(2)
        tot = kio.read_global_gmm_accs(f, True)
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.array_equal(tot[k], (acc1[k] + acc2[k]).astype(F32).astype(np.float64)), k
    assert tool("gmm-global-sum-accs").main(["sum.acc", "1.1.acc", "none.acc"]) == 255
    assert "dimension or flags mismatch, 9, 4, mvw vs. 9, 4, 5" in capfd.readouterr().err


def check_written(acc, restated, x):
    """The floats of a file against the restatement's doubles: each within the accumulation bound (n + 2) 2^-53 sum |t| of the
    exact sum (tests/gmm_acc_cases.py) plus the half ulp of the conversion to float the writer makes."""
    used, post = restated["used"], restated["post"]
    for k, xs in (("occ", None), ("mean_acc", x[used].astype(np.float64)), ("var_acc", x[used].astype(np.float64) ** 2)):
        p = np.abs(post.astype(np.float64))
        mag = p.sum(0) if xs is None else p.T @ np.abs(xs)
        bound = 2 * (len(used) + 2) * 2.0 ** -53 * mag + 2.0 ** -24 * np.abs(restated[k]) * (1 + 2.0 ** -20)
        err = np.abs(acc[k] - restated[k])
        print(k, "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), k


def test_job_refusal_under_world_2(files, monkeypatch, capfd):
    monkeypatch.chdir(files["dir"])
    assert tool("gmm-gselect").main(["--world=2", "--rank=1", "0.dubm", "ark:feats.ark", "ark:all.gselect.ark"]) == 255
    assert "ERROR (gmm-gselect) --world=2: the gselect wspecifier needs JOB in its name" in capfd.readouterr().err
    assert tool("gmm-global-acc-stats").main(["--world=2", "--rank=1", "0.dubm", "ark:feats.ark", "all.acc"]) == 255
    assert "ERROR (gmm-global-acc-stats) --world=2: the statistics file needs JOB in its name" in capfd.readouterr().err
    assert tool("gmm-global-sum-accs").main(["--world=2", "--rank=0", "all.acc", "1.JOB.acc", "2.JOB.acc"]) == 255
    assert "ERROR (gmm-global-sum-accs) --world=2: the output needs JOB in its name" in capfd.readouterr().err
    assert not (files["dir"] / "all.acc").exists() and not (files["dir"] / "all.gselect.ark").exists()
