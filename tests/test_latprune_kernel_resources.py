"""Compile-only guard (no GPU: hipcc cross-compiles): the kernels of csrc/kh_latprune.hip keep their per-lane state in
registers - no scratch, no spills - at the library's own flags, which must keep contraction and fast-math off (the
bit-exactness of the pruning decisions depends on them).  The register count is recorded in DESIGN.md, not asserted."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_prune_kernels_have_no_scratch(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_latprune.hip")
    assert "-ffp-contract=off" in build.FLAGS and "-fno-fast-math" in build.FLAGS
    p = subprocess.run([HIPCC] + build.FLAGS + build.EXTRA.get("kh_latprune.hip", []) +
                       ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    n_kernels = len(re.findall(r"^__global__", open(src).read(), flags=re.M))
    assert n_kernels >= 1 and len(names) == n_kernels and any("PruneKernel" in n for n in names), names
    get = lambda what: [int(x) for x in re.findall(re.escape(what) + r":\s*(\d+)", p.stderr)]
    assert get("ScratchSize [bytes/lane]") == [0] * n_kernels
    assert get("VGPRs Spill") == [0] * n_kernels and get("SGPRs Spill") == [0] * n_kernels
