"""Compile-only guard (no GPU: hipcc cross-compiles): the kernels of csrc/kh_lda.hip - LdaAccumulateKernel, LdaReduceKernel and
LdaFirstKernel - spill no register at the library's own flags, use no scratch and have no dynamic stack.
LdaAccumulateKernel's static LDS is the figure its header comment derives, at every D: the A image of 32 items at a pitch of
80 doubles and the B image at a pitch of 80 floats (32 x 80 x 8 + 32 x 80 x 4 = 30720 bytes).  Register counts and occupancy
are printed and recorded in DESIGN.md, not asserted.  Resource figures only: no instruction is looked at."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_lda_kernel_resources(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_lda.hip")
    text = open(src).read()
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    assert len(re.findall(r"^__global__", text, flags=re.M)) == 3 and len(names) == 3, names
    assert not any("ComponentPosteriorsKernel" in n for n in names), names       # the shared header's kernel is not compiled here
    for k in ("LdaAccumulateKernel", "LdaReduceKernel", "LdaFirstKernel"):
        assert sum(k in n for n in names) == 1, names
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    print("kernels", names, "VGPRs", get("VGPRs"), "AGPRs", get("AGPRs"), "SGPRs", get("SGPRs"), "LDS", get("LDS Size [bytes/block]"),
          "scratch", get("ScratchSize [bytes/lane]"), "occupancy", get("Occupancy [waves/SIMD]"))
    assert get("VGPRs Spill") == [0] * 3 and get("SGPRs Spill") == [0] * 3
    assert p.stderr.count("Dynamic Stack: False") == 3
    assert get("ScratchSize [bytes/lane]") == [0] * 3
    lds = dict(zip(names, get("LDS Size [bytes/block]")))
    # the figure of the header comment, and the constants it is made of
    m = re.search(r"(\d+) x (\d+) x 8 \+ (\d+) x (\d+) x 4 = (\d+) bytes", text)
    assert m and int(m.group(1)) * int(m.group(2)) * 8 + int(m.group(3)) * int(m.group(4)) * 4 == int(m.group(5)) == 30720
    assert m.group(1) == m.group(3) and re.search(r"constexpr int kSub = %s;" % m.group(1), text)
    assert re.search(r"constexpr int kAs = %s;" % m.group(2), text) and re.search(r"constexpr int kBs = %s;" % m.group(4), text)
    assert [v for n, v in lds.items() if "LdaAccumulateKernel" in n] == [30720]
    assert [v for n, v in lds.items() if "LdaAccumulateKernel" not in n] == [0, 0]
