"""Compile-only pin of the reference-order decode kernel's scratch (no GPU: hipcc cross-compiles).

Scratch is traffic: a spilled register of a persistent 1024-thread workgroup is 4 KB per store and per
load from a working set no cache holds.  Round 7 took `DecodeKernel<true, true>` from 116 B per lane / 15 static scratch
loads to 24 B / 5: all but two of the loads were the running-cutoff scan's per-lane state (sixteen counts + sixteen M
words in the 16-bit tier, eight + eight in the first) spilled around the scan's barrier; the counts now cross it as the
16-bit pairs they arrive in, and the M words are read again behind it.

The goal was 24 B / 4 loads.  The bytes are met; the loads are 5, one above the goal: the five that are left are five of
the 16-bit tier's eight packed count words, one dword each, stored in front of the scan's block primitive and loaded in
the loop behind it.  They cannot be read again from LDS instead: behind the barrier the lanes write the scan's results
over the very words the counts came from.  Hence the pin below: 24 B (a multiple of 8 already) and 5 loads + 1."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_reference_order_kernel_scratch():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_mix.py"), "kh_decoder.hip"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = {}
    for line in p.stdout.splitlines():
        m = re.match(r"^(.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = [int(x) for x in m.groups()[1:]]
    # columns: instructions, readlane, writelane, scratch loads, scratch stores, scratch bytes, bpermute, dpp
    x = rows[next(k for k in rows if "DecodeKernel<true, true>" in k)]
    assert x[5] <= 24 and x[3] <= 6, "DecodeKernel<1,1> scratch %d B per lane, %d static scratch loads (24 B / 5 in round 7; 116 / 15 before)" % (x[5], x[3])
    c = rows[next(k for k in rows if "DecodeKernel<true, false>" in k)]
    assert c[5] == 0 and c[3] == 0, "DecodeKernel<1,0> scratch %d B per lane, %d static scratch loads (0 / 0 since round 6)" % (c[5], c[3])
