"""CPU: bin/sum-lda-accs (tools/sum_lda_accs.py) needs no device: two job files summed equal the restatement's
Read(add = true) of each followed by Write, byte for byte (tests/lda_restatement.py); "-" is standard output; usage and exit
status 1 with fewer than two arguments; the mismatch message of Read."""
import os
import subprocess
import sys

import numpy as np

import lda_restatement as L
from conftest import ROOT


def job_acc(seed, nc=4, dim=6):
    rng = np.random.default_rng(seed)
    acc = L.init(L.empty(), nc, dim)
    for _ in range(80):
        L.accumulate(acc, (rng.standard_normal(dim) * 2 + 0.5).astype(np.float32), int(rng.integers(1, nc)), rng.random() + 0.25)
    return acc                                                               # class 0 has no count


def run(d, *args):
    env = dict(os.environ, PATH=os.path.join(ROOT, "bin") + os.pathsep + os.environ["PATH"], PYTHON=sys.executable, HIP_VISIBLE_DEVICES="")
    return subprocess.run(["sum-lda-accs"] + list(args), cwd=d, env=env, capture_output=True, timeout=120)


def test_two_job_files(tmp_path):
    a, b = job_acc(1), job_acc(2)
    (tmp_path / "lda.1.acc").write_bytes(b"\0B" + L.write(a, True))
    (tmp_path / "lda.2.acc").write_bytes(b"\0B" + L.write(b, True))
    lda = L.read_of_write(a, L.empty())                                      # LdaEstimate lda; lda.Read(..., add = true) twice
    lda = L.read_of_write(b, lda)
    p = run(tmp_path, "lda.acc", "lda.1.acc", "lda.2.acc")
    assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "lda.acc").read_bytes() == b"\0B" + L.write(lda, True)
    p = run(tmp_path, "--binary=false", "-", "lda.1.acc", "lda.2.acc")
    assert p.returncode == 0 and p.stdout == L.write(lda, False)
    # one input: Read(Write(a)) written again
    p = run(tmp_path, "-", "lda.2.acc")
    assert p.returncode == 0 and p.stdout == b"\0B" + L.write(L.read_of_write(b), True)


def test_usage_and_mismatch(tmp_path):
    p = run(tmp_path, "only.acc")
    assert p.returncode == 1 and b"Usage: sum-lda-accs [options] <stats-out> <stats-in1> <stats-in2> ..." in p.stderr
    assert b"Sum stats obtained with acc-lda." in p.stderr and not (tmp_path / "only.acc").exists()
    (tmp_path / "a.acc").write_bytes(b"\0B" + L.write(job_acc(1), True))
    (tmp_path / "b.acc").write_bytes(L.write(job_acc(2, nc=5), False))       # a text file
    p = run(tmp_path, "bad.acc", "a.acc", "b.acc")
    assert p.returncode != 0 and b"LdaEstimate::Read, dimension or classes count mismatch, 4, 6,  vs. 5, 6" in p.stderr
