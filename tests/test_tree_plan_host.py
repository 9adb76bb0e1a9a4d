"""No GPU: the host plan of kh_tree_acc_stats (csrc/kh_tree_plan.h, no HIP in it) in a stand-alone program of its own
(tests/cpp/tree_plan_test.cc), built with plain g++ with and without -fsanitize=address,undefined and run directly: empty
input, every frame unused, one event holding everything, E events of one frame each, interleaved runs - the sort keeps
frame order within an event, the work list takes the longest runs first and covers every column block - and the refusals
with the documented messages."""
import os
import subprocess

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "sanitized"])
def test_tree_plan(tmp_path, flags):
    src = os.path.join(ROOT, "tests", "cpp", "tree_plan_test.cc")
    exe = str(tmp_path / "tree_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


def test_plan_header_has_no_hip():
    text = open(os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_tree_plan.h")).read()
    assert "#include <hip" not in text and "kh_common" not in text and "__global__" not in text and "__device__" not in text
