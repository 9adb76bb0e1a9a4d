"""CPU: bin/gmm-sum-accs (tools/gmm_acc_tools.py) needs no device: three job files summed equal the restated add
(gmm_acc_restatement.sum_accs: the files' floats added into doubles in argument order, written as floats); "-" is standard
output, as the recipes' "gmm-sum-accs - $dir/$x.*.acc |" needs; usage and exit status 1 with fewer than two arguments."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import gmm_acc_restatement as A
from conftest import ROOT, pkg


def make_acc(seed, flags=7):
    rng = np.random.default_rng(seed)
    off = np.array([0, 3, 4, 9], np.int32)
    return dict(occ=rng.random(9) * 100, mean_acc=rng.standard_normal((9, 5)) * 100 if flags & 1 else None,
                var_acc=rng.random((9, 5)) * 1000 if flags & 2 else None, pdf_offsets=off, dim=5, flags=flags,
                total_like=-float(rng.random()) * 1e4, total_frames=float(rng.integers(100, 200)), transition_accs=rng.random(7) * 50)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    kio = pkg("kaldi_io")
    d = tmp_path_factory.mktemp("sumaccs")
    accs = [make_acc(s) for s in (1, 2, 3)]
    for i, a in enumerate(accs):
        with open(d / ("%d.acc" % i), "wb") as f:
            if i != 1:
                f.write(b"\0B")
            kio.write_gmm_accs(f, a, binary=i != 1)               # the second file in text mode
    return d, accs


def run(d, *args):
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable, HIP_VISIBLE_DEVICES="")
    return subprocess.run(["gmm-sum-accs"] + list(args), cwd=d, env=env, capture_output=True, timeout=120)


def check_sum(got, accs):
    want = A.as_written(A.sum_accs(accs))
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.array_equal(got[k], want[k].astype(np.float64)), k
    assert np.array_equal(got["transition_accs"], want["transition_accs"])
    assert got["total_like"] == want["total_like"] and got["total_frames"] == want["total_frames"]


def test_three_files(files):
    d, accs = files
    kio = pkg("kaldi_io")
    text_like = kio.read_kaldi_object(str(d / "1.acc"), kio.read_gmm_accs)          # what the text file holds: 7 significant digits
    p = run(d, "sum.acc", "0.acc", "1.acc", "2.acc")
    assert p.returncode == 0, p.stderr[-2000:]
    err = p.stderr.decode()
    assert "LOG (gmm-sum-accs:main()) Summed 3 stats, total count " in err and "LOG (gmm-sum-accs:main()) Written stats to sum.acc" in err
    assert "LOG (gmm-sum-accs:main()) Total count of stats is " in err
    data = (d / "sum.acc").read_bytes()
    assert data[:2] == b"\0B"
    check_sum(kio.read_gmm_accs(io.BytesIO(data[2:]), True), [accs[0], text_like, accs[2]])


def test_dash_is_standard_output_and_text_mode(files):
    d, accs = files
    kio = pkg("kaldi_io")
    p = run(d, "-", "0.acc", "2.acc")
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout[:2] == b"\0B"
    check_sum(kio.read_gmm_accs(io.BytesIO(p.stdout[2:]), True), [accs[0], accs[2]])
    p = run(d, "--binary=false", "-", "0.acc", "2.acc")
    assert p.returncode == 0 and p.stdout.startswith(b" [ ") and b"<NUMPDFS> 3 <GMMACCS> <VECSIZE> 5 " in p.stdout
    got = kio.read_gmm_accs(io.BytesIO(p.stdout), False)
    assert np.allclose(got["occ"], A.sum_accs([accs[0], accs[2]])["occ"], rtol=1e-6)


def test_usage_and_mismatch(files):
    d, accs = files
    p = run(d, "only.acc")
    assert p.returncode == 1 and b"Usage: gmm-sum-accs [options] <stats-out> <stats-in1> <stats-in2> ..." in p.stderr
    assert not (d / "only.acc").exists()
    kio = pkg("kaldi_io")
    with open(d / "mw.acc", "wb") as f:
        f.write(b"\0B")
        kio.write_gmm_accs(f, make_acc(4, flags=5), True)
    p = run(d, "bad.acc", "0.acc", "mw.acc")
    assert p.returncode != 0 and b"dimension or flags mismatch, 3, 5, mvw vs. 3, 5, 5" in p.stderr
