"""tools/gmm_acc_cpu_baseline.cc - the one-thread host program tools/gmm_acc_rate.py times next to the device route - compiles,
also under -fsanitize=address,undefined (a stand-alone program: no report, the same outputs), and agrees with
tests/gmm_acc_restatement.py: the posteriors and scores within the A1 bounds of tests/fmllr_cases.py (the host libm's expf /
logf are within 1 ulp, as the device's), the accumulators bit for bit on its own posteriors (both add the entries in frame
order, a product and an addition each, uncontracted).  No device."""
import subprocess

import numpy as np
import pytest

import fmllr_cases as FC
import gmm_acc_cases as C
import gmm_acc_restatement as A

SAN = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.gmm_acc_rate as rate
    d = tmp_path_factory.mktemp("gmm_acc_cpu")
    san = d / "san"
    san.mkdir()
    return rate, rate.cpu_baseline(str(d)), rate.cpu_baseline(str(san), SAN), str(d)


@pytest.fixture(scope="module")
def job(oracle):
    am, tid2pdf, utts = C.e2e_utterances(oracle)
    feats = np.concatenate([m for _, m, _, _ in utts[:2]])
    posts = [fr for _, _, p, _ in utts[:2] for fr in p]
    ent = A.R.entries_of(A.convert_posterior_to_pdfs(tid2pdf, posts), am["pdf_offsets"])
    post, like = A.R.component_posteriors(am, feats, ent)
    return am, feats, ent, post, like


def check(got, am, feats2, ent, post, like, flags):
    assert (np.abs(got["post"].astype(np.float64) - post) <= FC.post_bound(post, ent["goff"])).all()
    assert (np.abs(got["like"].astype(np.float64) - like) <= FC.like_bound(like, ent["goff"])).all()
    want = A.accumulate_entries(A.init_accs(am["pdf_offsets"], feats2.shape[1], flags), feats2, ent, got["post"], got["like"])
    for k in ("occ", "mean_acc", "var_acc"):
        if want[k] is None:
            assert not got[k].any(), k
        else:
            assert np.array_equal(got[k], want[k]), k
    assert got["total_like"] == want["total_like"] and got["total_frames"] == want["total_frames"]


def test_baseline_agrees_with_the_restatement(rate, job):
    rate, exe, exe_san, d = rate
    am, feats, ent, post, like = job
    got, ms = rate.run_cpu(exe, am, feats, feats, ent, 7, d)
    assert len(ms) == 2
    check(got, am, feats, ent, post, like, 7)
    san, _ = rate.run_cpu(exe_san, am, feats, feats, ent, 7, d)          # the sanitized build: the same bytes out, nothing reported
    for k in got:
        assert np.array_equal(got[k], san[k]), k


def test_baseline_two_features_and_flags(rate, job):
    rate, exe, exe_san, d = rate
    am, feats, ent, post, like = job
    feats2 = C.second_features(feats, 9, 3)
    got, _ = rate.run_cpu(exe_san, am, feats, feats2, ent, 7, d)
    assert got["mean_acc"].shape == (28, 9)
    check(got, am, feats2, ent, post, like, 7)
    got, _ = rate.run_cpu(exe_san, am, feats, feats, ent, 5, d)
    check(got, am, feats, ent, post, like, 5)


def test_baseline_refuses_bad_input(rate, tmp_path):
    rate, exe, exe_san, d = rate
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\0" * 16)
    p = subprocess.run([exe_san, str(bad), str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 2 and "short input" in p.stderr


def test_kernel_bytes_of_the_rate_tool(rate):
    """The traffic figure of tools/gmm_acc_rate.py on a case small enough to count by hand: pdfs of 3 and 17 Gaussians with 2
    and 300 entries, D = 5, chunk 256."""
    rate = rate[0]
    ent = dict(pdf=np.array([0] * 2 + [1] * 300, np.int32))
    acc, red = rate.kernel_bytes([0, 3, 20], ent, 5, 256)
    assert acc == 2 * 1 * (20 + 12) + 2 * 3 * 4 + 300 * 2 * (20 + 12) + 300 * 17 * 4
    assert red == 1 * 3 * 11 * 8 + 2 * 17 * 11 * 8
