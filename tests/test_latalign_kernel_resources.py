"""Compile-only guard (no GPU: hipcc cross-compiles): AlignKernel of csrc/kh_latalign.hip, the one kernel of the file, spills
no register at the library's own flags and has no dynamic stack.  Its candidate descriptor (a few pointers and lengths per
lane) is what the compiler keeps in LDS and scratch; both are bounded here.  The register count is recorded in DESIGN.md,
not asserted."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_align_kernel_resources(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_latalign.hip")
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    n_kernels = len(re.findall(r"^__global__", open(src).read(), flags=re.M))
    assert n_kernels == 1 and len(names) == 1 and "AlignKernel" in names[0], names
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    print("VGPRs", get("VGPRs"), "SGPRs", get("SGPRs"), "LDS", get("LDS Size [bytes/block]"), "scratch", get("ScratchSize [bytes/lane]"))
    assert get("VGPRs Spill") == [0] and get("SGPRs Spill") == [0]
    assert "Dynamic Stack: False" in p.stderr
    assert get("ScratchSize [bytes/lane]")[0] <= 64 and get("LDS Size [bytes/block]")[0] <= 8192
    assert get("Occupancy [waves/SIMD]")[0] >= 2
