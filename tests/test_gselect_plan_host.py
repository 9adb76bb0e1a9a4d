"""No GPU: the host side of kh_gmm_gselect and kh_gmm_preselect_posteriors (csrc/kh_gselect_plan.h, no HIP in it) in a
stand-alone program of its own (tests/cpp/gselect_plan_test.cc), built with plain g++ with and without
-fsanitize=address,undefined and run directly: no frame, lists that share Gaussians across frames, frames of weight 0 whose
lists are not looked at, the used frames, the row chunks - and every refusal with its documented message."""
import os
import subprocess

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SRC = os.path.join(ROOT, "tests", "cpp", "gselect_plan_test.cc")

REFUSALS = {
    "first": "sel_offsets[0] = 1, not 0",
    "backwards": "sel_offsets runs backwards at frame 1",
    "negative": "frame 1 lists Gaussian -1, the model has 4",
    "range": "frame 1 lists Gaussian 4, the model has 4",
    "empty": "frame 1 has an empty list",
    "twice": "frame 1 lists Gaussian 2 twice",
    "long": "frame 1 lists 3 Gaussians, at most 2",
}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gselect_plan") / "gselect_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", SRC, "-o", exe])
    return exe


def test_gselect_plan_plain(plain):
    r = subprocess.run([plain], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


def test_gselect_plan_sanitized(tmp_path):
    exe = str(tmp_path / "gselect_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + SAN + [SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_message(plain, name):
    r = subprocess.run([plain, name], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.rstrip("\n") == REFUSALS[name], r.stdout


def test_plan_header_has_no_hip():
    text = open(os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_gselect_plan.h")).read()
    assert "#include <hip" not in text and "kh_common" not in text and "__global__" not in text and "__device__" not in text
