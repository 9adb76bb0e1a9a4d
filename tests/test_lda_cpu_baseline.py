"""tools/lda_cpu_baseline.cc - the one-thread host program tools/lda_rate.py times next to the device route - compiles, also
under -fsanitize=address,undefined (a stand-alone program: no report, the same outputs), and agrees with
tests/lda_restatement.py on small cases: after the same srand the same pruned weights bit for bit; the three statistics
within the summation bound of tests/lda_cases.py of the exact sums, and equal to the restatement's bit for bit (both add the
items in order, a product and an addition each, uncontracted).  No device."""
import subprocess

import numpy as np
import pytest

import lda_cases as C
import lda_restatement as L
import mllt_restatement as M

SAN = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.lda_rate as rate
    d = tmp_path_factory.mktemp("lda_cpu")
    san = d / "san"
    san.mkdir()
    return rate, rate.cpu_baseline(str(d)), rate.cpu_baseline(str(san), SAN), str(d)


@pytest.mark.parametrize("dim,prune", [(5, 0.0), (5, 0.25), (5, 4.0), (17, 0.5)])
def test_baseline_agrees_with_the_restatement(rate, dim, prune):
    rate, exe, exe_san, d = rate
    c = C.kernel_case(dim, 60, 8)
    ent, nc = c["ent"], c["num_classes"]
    got, ms = rate.run_cpu(exe, c["feats"], ent, nc, prune, 99, d)
    assert len(ms) == 2
    M.srand(99)
    pruned = np.array([M.rand_prune(v, prune) for v in ent["weight"]], np.float32)
    assert np.array_equal(got["pruned"].view(np.int32), pruned.view(np.int32))
    assert got["items"] == int((pruned != 0).sum()) and (got["items"] == 60) == (prune == 0.0)
    ref = C.restate(c["feats"], dict(ent, weight=pruned), nc)
    for k in ("zero", "first", "second"):
        assert np.array_equal(got[k], ref[k]), k
    x, w, cls = C.items_of(c["feats"], dict(ent, weight=pruned))
    acc = dict(got, dim=dim, num_classes=nc)
    print("rand_prune", prune, "items", len(w), "baseline worst error / bound", C.check_bound(acc, x, w, cls, 0, "baseline"))
    san, _ = rate.run_cpu(exe_san, c["feats"], ent, nc, prune, 99, d)        # the sanitized build: the same bytes out
    for k in ("pruned", "zero", "first", "second"):
        assert np.array_equal(got[k], san[k]), k
    assert L.write(dict(ref, dim=dim, num_classes=nc), True) == L.write(acc, True)


def test_baseline_refuses_bad_input(rate, tmp_path):
    rate, exe, exe_san, d = rate
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\0" * 16)
    p = subprocess.run([exe_san, str(bad), str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 2 and "short input" in p.stderr
    import struct
    bad.write_bytes(struct.pack("<5if", 1, 2, 3, 1, -1, 0.0) + np.zeros(2, "<f4").tobytes() + np.array([0, 1], "<i8").tobytes()
                    + np.array([3], "<i4").tobytes() + np.ones(1, "<f4").tobytes())
    p = subprocess.run([exe_san, str(bad), str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 2 and "inconsistent offsets" in p.stderr          # pdf 3 of 3 classes
