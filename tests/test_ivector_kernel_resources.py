"""Compile-only guard (no GPU: hipcc cross-compiles): the static LDS of the iVector kernels that also take model-sized
dynamic LDS is what csrc/kh_ivector.hip's host code assumes when it refuses a model that would not fit (static + dynamic
<= kLdsLimit, named constants beside the __shared__ declarations), and no iVector kernel uses scratch memory - at the
library's own flags."""
import os
import re
import subprocess

import ivector_cases as C
from conftest import pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ASSUMED = {"IvSolveKernel": "kSolveStaticLds", "IvStreamKernel": "kStreamStaticLds", "IvStatsKernel": "kStatsStaticLds",
           "IvLinKernel": "kLinStaticLds"}


def test_static_lds_is_within_what_the_host_assumes_and_no_kernel_uses_scratch(tmp_path):
    build = pkg("build")
    p = subprocess.run([HIPCC] + build.flags_for(C.HIP_SOURCE) + ["-Rpass-analysis=kernel-resource-usage", "-c", C.HIP_SOURCE, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    # one block of remarks per kernel: "Function Name: <mangled>" followed by its figures
    blocks = re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]
    res = {}
    for b in blocks:
        mangled = b.split()[0]
        mo = re.search(r"\d+(Iv[A-Za-z0-9]+Kernel)", mangled)
        if not mo:
            continue
        get = lambda what: int(re.search(re.escape(what) + r":\s*(\d+)", b).group(1))
        res[mo.group(1)] = dict(lds=get("LDS Size [bytes/block]"), scratch=get("ScratchSize [bytes/lane]"))
    print(res)
    kernels = set(re.findall(r"\b(Iv[A-Za-z0-9]+Kernel)\(", open(C.HIP_SOURCE).read()))
    assert kernels == set(res) and len(kernels) >= 13, (sorted(kernels), sorted(res))     # every kernel of the file was seen
    K = C.kernel_constants()
    for name, const in ASSUMED.items():
        assert res[name]["lds"] <= K[const], (name, res[name]["lds"], K[const])
        assert res[name]["lds"] > 0
    for name, r in res.items():
        assert r["scratch"] == 0, (name, r)
    # the kernels the host launches without an LDS check hold only what their arrays of fixed size need
    for name in set(res) - set(ASSUMED):
        assert res[name]["lds"] <= K["kLdsLimit"], (name, res[name])
