"""Compile-only guard (no GPU: hipcc cross-compiles): the best-path kernel of csrc/kh_latbest.hip keeps its per-lane state
in registers - no scratch, no spills, no LDS - at the library's own flags."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_best_path_kernel_has_no_scratch(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_latbest.hip")
    p = subprocess.run([HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "-ffp-contract=off" in build.FLAGS and "-fno-fast-math" in build.FLAGS       # the bit-exactness depends on them
    assert "BestPathKernel" in p.stderr
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    assert get("ScratchSize [bytes/lane]") == [0] and get("VGPRs Spill") == [0] and get("SGPRs Spill") == [0]
    assert get("LDS Size [bytes/block]") == [0]
    assert get("VGPRs")[0] <= 64, "the recorded build uses 56 vector registers (8 waves per SIMD by the register budget)"
