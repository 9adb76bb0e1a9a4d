"""Compile-only guard (no GPU: hipcc cross-compiles): the two kernels of csrc/kh_latrescore.hip use no scratch at the
library's own flags.  Nothing else is inspected; the register counts are printed."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_rescore_kernels_use_no_scratch(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_latrescore.hip")
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    n_kernels = len(re.findall(r"^__global__", open(src).read(), flags=re.M))
    assert n_kernels == 2 and len(names) == 2 and any("RescoreShortKernel" in n for n in names) and any("RescoreLongKernel" in n for n in names), names
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    print("VGPRs", get("VGPRs"), "SGPRs", get("SGPRs"), "scratch", get("ScratchSize [bytes/lane]"))
    assert get("ScratchSize [bytes/lane]") == [0, 0]
