"""Compile-only guard (no GPU: hipcc cross-compiles): AlignKernel of csrc/kh_align.hip, the one kernel of the file, spills no
register at the library's own flags, has no dynamic stack and no scratch.  Its static LDS is the reduction arrays only
(256 doubles + 256 int32 = 3072 bytes; DESIGN.md "Forced alignment"); the token costs are dynamic LDS sized per launch.
The register counts are printed and recorded in DESIGN.md, not asserted."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_align_compiled_kernel_resources(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_align.hip")
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    n_kernels = len(re.findall(r"^__global__", open(src).read(), flags=re.M))
    assert n_kernels == 1 and len(names) == 1 and "AlignKernel" in names[0], names
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    print("VGPRs", get("VGPRs"), "SGPRs", get("SGPRs"), "LDS", get("LDS Size [bytes/block]"), "scratch", get("ScratchSize [bytes/lane]"),
          "occupancy", get("Occupancy [waves/SIMD]"))
    assert get("VGPRs Spill") == [0] and get("SGPRs Spill") == [0]
    assert "Dynamic Stack: False" in p.stderr
    assert get("ScratchSize [bytes/lane]") == [0]
    assert get("LDS Size [bytes/block]")[0] <= 3072
