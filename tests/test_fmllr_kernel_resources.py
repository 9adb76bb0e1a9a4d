"""Compile-only guard (no GPU: hipcc cross-compiles): the four kernels of csrc/kh_fmllr.hip spill no register at the library's
own flags, use no scratch and have no dynamic stack.  FmllrAccumulateKernel's static LDS is the x+ image and the a / b image of
32 merged frames (32 x 65 + 2 x 32 x 64 floats = 24704 bytes).  Register counts are printed and recorded in DESIGN.md, not
asserted."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_fmllr_kernel_resources(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_fmllr.hip")
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    # three kernels of its own and the shared posterior kernel (csrc/kh_gmmstats.h), of which it compiles <false> alone
    text = open(src).read() + open(os.path.join(os.path.dirname(src), "kh_gmmstats.h")).read()
    n_kernels = len(re.findall(r"^__global__", text, flags=re.M))
    assert n_kernels == 4 and len(names) == 4, names
    for k in ("ComponentPosteriorsKernelILb0EE", "FrameStatsKernel", "FmllrAccumulateKernel", "FmllrReduceKernel"):
        assert sum(k in n for n in names) == 1, k
    assert "atomic" not in re.sub(r"//.*", "", text)
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    print("VGPRs", get("VGPRs"), "AGPRs", get("AGPRs"), "SGPRs", get("SGPRs"), "LDS", get("LDS Size [bytes/block]"),
          "scratch", get("ScratchSize [bytes/lane]"), "occupancy", get("Occupancy [waves/SIMD]"))
    assert get("VGPRs Spill") == [0] * 4 and get("SGPRs Spill") == [0] * 4
    assert p.stderr.count("Dynamic Stack: False") == 4
    assert get("ScratchSize [bytes/lane]") == [0] * 4
    lds = dict(zip(names, get("LDS Size [bytes/block]")))
    assert [v for n, v in lds.items() if "FmllrAccumulateKernel" in n] == [24704]
    assert all(v == 0 for n, v in lds.items() if "FmllrAccumulateKernel" not in n)
