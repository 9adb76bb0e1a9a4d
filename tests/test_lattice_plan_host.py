"""No GPU: the host sizing of the lattice kernels (csrc/kh_lattice_plan.h, no HIP in it) in a stand-alone program of its own
(tests/cpp/lattice_plan_test.cc), built with plain g++ with and without -fsanitize=address,undefined and run directly:
workgroups per CU, windows, LDS-resident states and staging at the batch sizes 1, 256, 257, 512, 513, 768, 769 and 5000 on 256
CUs; the window is the smallest power of two that holds the largest lattice, within [512, cap]; KH_LATTICE_WIN is taken only
for a power of two in [512, 16384]; the workgroups that share a CU fit its 160 KB; every window the plan can choose keeps
"the wave that wrote a slot rewrites it"."""
import os
import subprocess

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "sanitized"])
def test_lattice_plan(tmp_path, flags):
    src = os.path.join(ROOT, "tests", "cpp", "lattice_plan_test.cc")
    exe = str(tmp_path / "lattice_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


def test_plan_header_has_no_hip():
    text = open(os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_lattice_plan.h")).read()
    assert "#include <hip" not in text and "kh_common" not in text and "__global__" not in text and "__device__" not in text
