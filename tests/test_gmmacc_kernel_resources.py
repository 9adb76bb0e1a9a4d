"""Compile-only guard (no GPU: hipcc cross-compiles): the three kernels of csrc/kh_gmmacc.hip spill no register at the library's
own flags, use no scratch and have no dynamic stack.  GmmAccumulateKernel's static LDS is the figure its header comment
derives: the x image of 32 entries at a pitch of 144 floats and their 16 posteriors (32 x 144 x 4 + 32 x 16 x 4 = 20480
bytes).  Register counts are printed and recorded in DESIGN.md, not asserted."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_gmmacc_kernel_resources(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_gmmacc.hip")
    text = open(src).read()
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    # two kernels of its own and the shared posterior kernel (csrc/kh_gmmstats.h), of which it compiles <true> alone
    shared = open(os.path.join(os.path.dirname(src), "kh_gmmstats.h")).read()
    n_kernels = len(re.findall(r"^__global__", text + shared, flags=re.M))
    assert n_kernels == 3 and len(names) == 3, names
    for k in ("ComponentPosteriorsKernelILb1EE", "GmmAccumulateKernel", "GmmAccReduceKernel"):
        assert sum(k in n for n in names) == 1, k
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    print("kernels", names, "VGPRs", get("VGPRs"), "AGPRs", get("AGPRs"), "SGPRs", get("SGPRs"), "LDS", get("LDS Size [bytes/block]"),
          "scratch", get("ScratchSize [bytes/lane]"), "occupancy", get("Occupancy [waves/SIMD]"))
    assert get("VGPRs Spill") == [0] * 3 and get("SGPRs Spill") == [0] * 3
    assert p.stderr.count("Dynamic Stack: False") == 3
    assert get("ScratchSize [bytes/lane]") == [0] * 3
    lds = dict(zip(names, get("LDS Size [bytes/block]")))
    # the figure of the header comment, and the constants it is made of
    m = re.search(r"(\d+) x (\d+) x 4 \+ (\d+) x 16 x 4 = (\d+) bytes", text)
    assert m and int(m.group(1)) * int(m.group(2)) * 4 + int(m.group(3)) * 16 * 4 == int(m.group(4)) == 20480
    assert re.search(r"constexpr int kSub = %s;" % m.group(1), text) and re.search(r"constexpr int kXs = %s;" % m.group(2), text)
    assert [v for n, v in lds.items() if "GmmAccumulateKernel" in n] == [20480]
    assert [v for n, v in lds.items() if "GmmAccumulateKernel" not in n] == [0, 0]
    assert "atomic" not in re.sub(r"//.*", "", text + shared)
