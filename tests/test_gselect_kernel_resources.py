"""Compile-only guard (no GPU: hipcc cross-compiles): the kernels of csrc/kh_gselect.hip - GselectKernel and
PreselectPosteriorsKernel, each in its small and its large form - spill no register at the library's own flags, use no scratch
and have no dynamic stack; their static LDS is the figure the header comment derives: the waves' score rows, 4 x 512 x 4 = 8192
bytes (small) and 2 x 4096 x 4 = 32768 bytes (large).  The source names no atomic operation.  Register counts and occupancy
are printed, not asserted.  Resource figures only: no instruction is looked at."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_gselect_kernel_resources(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_gselect.hip")
    text = open(src).read()
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    assert len(re.findall(r"^__global__", text, flags=re.M)) == 2 and len(names) == 4, names
    assert sum("GselectKernel" in n for n in names) == 2 and sum("PreselectPosteriorsKernel" in n for n in names) == 2
    code = re.sub(r"//.*", "", text + open(os.path.join(os.path.dirname(src), "kh_gselect_plan.h")).read())
    assert "atomic" not in code.lower()
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    print("kernels", names)
    print("VGPRs", get("VGPRs"), "AGPRs", get("AGPRs"), "SGPRs", get("SGPRs"), "LDS", get("LDS Size [bytes/block]"),
          "scratch", get("ScratchSize [bytes/lane]"), "occupancy", get("Occupancy [waves/SIMD]"))
    assert get("VGPRs Spill") == [0] * 4 and get("SGPRs Spill") == [0] * 4
    assert p.stderr.count("Dynamic Stack: False") == 4
    assert get("ScratchSize [bytes/lane]") == [0] * 4
    # the figures of the header comment, and the constants they are made of
    m = re.search(r"(\d+) x (\d+) x 4 = (\d+) bytes and (\d+) x (\d+) x 4 = (\d+) bytes", text)
    assert m
    sw, sc, sb, bw, bc, bb = (int(x) for x in m.groups())
    assert sw * sc * 4 == sb == 8192 and bw * bc * 4 == bb == 32768
    assert re.search(r"constexpr int kSmallCap = %d, kSmallWaves = %d;" % (sc, sw), text)
    assert re.search(r"constexpr int kMaxGauss = %d;" % bc, text) and re.search(r"constexpr int kBigWaves = %d;" % bw, text)
    lds = dict(zip(names, get("LDS Size [bytes/block]")))
    for n, v in lds.items():
        assert v == (sb if "ILi%dE" % sc in n else bb), (n, v)
