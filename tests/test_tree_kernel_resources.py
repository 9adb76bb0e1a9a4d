"""Compile-only guard (no GPU: hipcc cross-compiles): the one kernel of csrc/kh_tree.hip, TreeAccumulateKernel, spills no
register at the library's own flags, uses no scratch and has no dynamic stack; its static LDS is the figure its header comment
derives, at every D: a tile of 32 rows at a pitch of 64 floats and the tile's 32 frame indices (32 x 64 x 4 + 32 x 4 = 8320 bytes).  The source names no atomic
operation: the sums are plain chains.  Register counts and occupancy are printed and recorded in DESIGN.md, not asserted.
Resource figures only: no instruction is looked at."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_tree_kernel_resources(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_tree.hip")
    text = open(src).read()
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    assert len(re.findall(r"^__global__", text, flags=re.M)) == 1 and len(names) == 1 and "TreeAccumulateKernel" in names[0], names
    code = re.sub(r"//.*", "", text + open(os.path.join(os.path.dirname(src), "kh_tree_plan.h")).read())
    assert "atomic" not in code.lower()
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    print("VGPRs", get("VGPRs"), "AGPRs", get("AGPRs"), "SGPRs", get("SGPRs"), "LDS", get("LDS Size [bytes/block]"),
          "scratch", get("ScratchSize [bytes/lane]"), "occupancy", get("Occupancy [waves/SIMD]"))
    assert get("VGPRs Spill") == [0] and get("SGPRs Spill") == [0]
    assert p.stderr.count("Dynamic Stack: False") == 1
    assert get("ScratchSize [bytes/lane]") == [0]
    # the figure of the header comment, and the constants it is made of
    m = re.search(r"(\d+) x (\d+) x 4 \+ (\d+) x 4 = (\d+) bytes", text)
    assert m and int(m.group(1)) * int(m.group(2)) * 4 + int(m.group(3)) * 4 == int(m.group(4)) == 8320
    assert re.search(r"constexpr int kTile = %s;" % m.group(1), text) and m.group(2) == "64" and m.group(3) == m.group(1)
    assert get("LDS Size [bytes/block]") == [8320]
