"""tools/fmllr_cpu_baseline.cc - the one-thread host program tools/fmllr_rate.py times next to the device route - compiles, also
under -fsanitize=address,undefined (a stand-alone program: no report, the same outputs), and agrees with
tests/fmllr_restatement.py: A1 within the bounds of tests/fmllr_cases.py (the host libm's expf / logf are within 1 ulp, as the
device's), A2 bit for bit on its own posteriors, B bit for bit on its own a / b / count (both add the merged frames in order,
without contraction), C within the measured tolerance.  No device."""
import numpy as np
import pytest

import fmllr_cases as C
import fmllr_restatement as R


@pytest.fixture(scope="module")
def rate(tmp_path_factory):
    import tools.fmllr_rate as rate
    d = tmp_path_factory.mktemp("fmllr_cpu")
    san = d / "san"
    san.mkdir()
    return rate, rate.cpu_baseline(str(d)), rate.cpu_baseline(str(san), ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), str(d)


@pytest.fixture(scope="module")
def e2e(oracle):
    return C.e2e_reference(oracle, types=["full"])


@pytest.mark.parametrize("update_type", C.TYPES)
def test_baseline_agrees_with_the_restatement(rate, e2e, update_type):
    rate, exe, exe_san, d = rate
    am, feats, utt, spk, posts, tid2pdf = e2e["case"]
    ent = e2e["ent"]
    got, ms = rate.run_cpu(exe, am, feats, utt, spk, ent, update_type, C.E2E_MIN_COUNT, 40, d)
    assert len(ms) == 4
    assert (np.abs(got["post"].astype(np.float64) - e2e["post"]) <= C.post_bound(e2e["post"], ent["goff"])).all()
    assert (np.abs(got["like"].astype(np.float64) - e2e["like"]) <= C.like_bound(e2e["like"], ent["goff"])).all()
    fs = R.frame_stats(am, feats, utt, spk, ent, got["post"])
    assert got["run_row"].tolist() == fs["run_row"].tolist() and got["spk_run_offsets"].tolist() == fs["spk_run_offsets"].tolist()
    for k in ("a", "b"):
        assert np.array_equal(got[k].view(np.int32), fs[k].view(np.int32)), k
    assert np.array_equal(got["count"], fs["count"])
    stats = R.accumulate(feats, dict(fs, a=got["a"], b=got["b"], count=got["count"]))
    for k in ("beta", "K", "G"):
        assert np.array_equal(got[k], stats[k]), k
    W, impr, count = R.update(stats, update_type=update_type, min_count=C.E2E_MIN_COUNT, num_iters=40)
    assert (np.abs(got["W"].astype(np.float64) - W) <= C.transform_tolerance(W, update_type)).all()
    assert np.array_equal(got["count_f"], count) and np.allclose(got["impr"], impr, rtol=1e-4, atol=1e-3)
    if update_type == "full":
        # the sanitized build: the same bytes out, nothing reported
        san, _ = rate.run_cpu(exe_san, am, feats, utt, spk, ent, update_type, C.E2E_MIN_COUNT, 40, d)
        for k in got:
            assert np.array_equal(got[k], san[k]), k


def test_baseline_on_the_merging_case(rate, oracle):
    """Posteriors from A1 on the a2 case's frames: merged frames across utterances, not across speakers, a frame without entries."""
    rate, exe, exe_san, d = rate
    am, feats, utt, spk, gposts = C.a2_case(oracle)
    posts = [[(p, 0.5) for p, _ in fr] for fr in gposts]
    ent = R.entries_of(posts, am["pdf_offsets"])
    got, _ = rate.run_cpu(exe_san, am, feats, utt, spk, ent, "none", 1.0, 1, d)
    fs = R.frame_stats(am, feats, utt, spk, ent, got["post"])
    assert got["run_row"].tolist() == fs["run_row"].tolist() == [0, 1, 4, 7, 8, 10, 11, 12, 13, 14, 15, 16, 20, 21, 22, 23]
    assert np.array_equal(got["a"].view(np.int32), fs["a"].view(np.int32)) and np.array_equal(got["count"], fs["count"])


def test_baseline_refuses_bad_input(rate, tmp_path):
    rate, exe, exe_san, d = rate
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\0" * 16)
    import subprocess
    p = subprocess.run([exe_san, str(bad), str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 2 and "short input" in p.stderr
