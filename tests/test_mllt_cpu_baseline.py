"""tools/mllt_cpu_baseline.cc - the one-thread host program tools/mllt_rate.py times next to the device route - compiles, also
under -fsanitize=address,undefined (a stand-alone program: no report, the same outputs), and agrees with
tests/mllt_restatement.py on a tiny case: after the same srand the same pruned posteriors bit for bit and the same beta; G
within the summation bound of tests/mllt_cases.py of the exact sums, and equal to the restatement's bit for bit (both add the
items in order, a product and an addition each, uncontracted).  No device."""
import subprocess

import numpy as np
import pytest

import mllt_cases as C
import mllt_restatement as M

SAN = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.mllt_rate as rate
    d = tmp_path_factory.mktemp("mllt_cpu")
    san = d / "san"
    san.mkdir()
    return rate, rate.cpu_baseline(str(d)), rate.cpu_baseline(str(san), SAN), str(d)


@pytest.mark.parametrize("prune", [0.0, 0.25, 4.0])
def test_baseline_agrees_with_the_restatement(rate, prune):
    rate, exe, exe_san, d = rate
    c = C.kernel_case(5, 60, 8)
    am = dict(pdf_offsets=c["off"], means_invvars=c["mi"], inv_vars=c["iv"])
    got, ms = rate.run_cpu(exe, am, c["feats"], c["ent"], c["post"], prune, 99, d)
    assert len(ms) == 2
    M.srand(99)
    acc = M.init_accs(5, prune)
    acc["trace"] = []
    M.accumulate_entries(acc, am, c["feats"], c["ent"], c["post"])
    pruned = np.asarray(acc["trace"], np.float32)[:, 1]
    assert np.array_equal(got["pruned"].view(np.int32), pruned.view(np.int32))
    assert got["beta"] == acc["beta"] and got["items"] == int((pruned != 0).sum())
    assert np.array_equal(got["G"], acc["G"])
    o, w, _ = C.items_of(c["off"], c["mi"], c["iv"], c["feats"], c["ent"], pruned)
    print("rand_prune", prune, "items", len(o), "baseline worst error / bound", C.check_bound(got["G"], o, w, 5, 0, "baseline"))
    san, _ = rate.run_cpu(exe_san, am, c["feats"], c["ent"], c["post"], prune, 99, d)      # the sanitized build: the same bytes out
    for k in ("pruned", "G"):
        assert np.array_equal(got[k], san[k]), k
    assert san["beta"] == got["beta"]


def test_baseline_refuses_bad_input(rate, tmp_path):
    rate, exe, exe_san, d = rate
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\0" * 16)
    p = subprocess.run([exe_san, str(bad), str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 2 and "short input" in p.stderr
