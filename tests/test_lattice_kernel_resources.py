"""Compile-only guard (no GPU: hipcc cross-compiles): the static LDS of the dataflow lattice kernels of csrc/kh_lattice.hip
stays within what csrc/kh_lattice_plan.h reserves for it when it sizes their dynamic LDS - read from the compiler's
kernel-resource-usage remarks at the library's own flags."""
import os
import re
import subprocess

from conftest import ROOT, pkg

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PLAN_H = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_lattice_plan.h")


def _plan_constants(tmp_path):
    """The reserved figures as the plan header itself gives them (a host program that prints them)."""
    src = tmp_path / "consts.cc"
    src.write_text('#include <cstdio>\n#include "%s"\nusing namespace kh_latplan;\n'
                   'int main() { std::printf("%%d %%d %%d %%d %%d %%d\\n", kPrepStaticBytes, kStageLarge, kStageSmall, kLdsBytes,\n'
                   '                         SweepStageBytes(kStageLarge), SweepStageBytes(kStageSmall)); return 0; }\n' % PLAN_H)
    exe = str(tmp_path / "consts")
    subprocess.check_call(["g++", "-std=c++17", str(src), "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    return dict(prep=v[0], stage_large=v[1], stage_small=v[2], lds=v[3], stage_bytes={v[1]: v[4], v[2]: v[5]})


def test_dataflow_kernels_static_lds_within_the_plan(tmp_path):
    build = pkg("build")
    src = os.path.join(ROOT, "old-kaldi-git_amd", "csrc", "kh_lattice.hip")
    p = subprocess.run([HIPCC] + build.flags_for(src) + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lds = {}
    for chunk in p.stderr.split("Function Name: ")[1:]:
        name = chunk.split()[0]
        m = re.search(r"LDS Size \[bytes/block\]:\s*(\d+)", chunk)
        assert m, name
        lds[name] = int(m.group(1))
    c = _plan_constants(tmp_path)
    assert (c["prep"], c["stage_large"], c["stage_small"], c["lds"]) == (21 * 1024, 384, 192, 160 * 1024)

    def one(frag):   # the one kernel whose mangled name holds frag
        got = [v for k, v in lds.items() if frag in k]
        assert len(got) == 1, (frag, sorted(lds))
        return got[0]

    # (Itanium mangling: PrepKernelDF<false> = ...PrepKernelDFILb0EE..., ForwardBackwardDFKernel<false, 384> = ...ILb0ELi384EE...)
    for prof in (0, 1):   # the profiling twins are sized by the same plan
        prep = one("PrepKernelDFILb%dEE" % prof)
        print("PrepKernelDF<%d>: static LDS %d, reserved %d" % (prof, prep, c["prep"]))
        assert 0 < prep <= c["prep"]
        for stage in (c["stage_large"], c["stage_small"]):
            got = one("ForwardBackwardDFKernelILb%dELi%dEE" % (prof, stage))
            print("ForwardBackwardDFKernel<%d, %d>: static LDS %d, reserved %d" % (prof, stage, got, c["stage_bytes"][stage]))
            assert 0 < got <= c["stage_bytes"][stage]
