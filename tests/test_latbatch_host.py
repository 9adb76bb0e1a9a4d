"""No GPU: the host-only helpers the batched compact-lattice entry points share (csrc/kh_latbatch_host.h: incoming-arc
lists, the top-sort refusals and their texts, the chunk plan), in a stand-alone program of their own
(tests/cpp/latbatch_host_test.cc) built with plain g++ under -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_latbatch_host_helpers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "latbatch_host_test.cc")
    exe = str(tmp_path / "latbatch_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
