#!/bin/bash
# usage: tools/build_variant_abl.sh NAME  -> tools/libkh_exp_NAME.so, the decoder built from a PATCHED COPY of
# csrc/kh_decoder.hip (the source itself, and with it the hash the PMC record carries, stays as it is).
#   dup_arc    pass 1 loads every arc record twice (the second load hits L1): what a divergent 16-byte load costs
#   dup_store  pass 1 stores a candidate's four words twice: what a coalesced store instruction costs
#   dup_tok    pass 1 loads the token cost / state words twice
set -e
cd "$(dirname "$0")/.."
name=$1
P=old-kaldi-git_amd
python -c "import importlib; importlib.import_module('old-kaldi-git_amd.build').build()" >/dev/null
src=/tmp/kh_decoder_$name.hip
python3 - "$name" "$P/csrc/kh_decoder.hip" "$src" <<'PY'
import sys
name, a, b = sys.argv[1:]
s = open(a).read()
def rep(old, new):
    global s
    assert s.count(old) == 1, (old, s.count(old))
    s = s.replace(old, new)
if name == "dup_arc":
    rep("        c_arc[k] = p.rec[ai];\n",
        "        c_arc[k] = p.rec[ai];\n        { int ai2 = ai; asm volatile(\"\" : \"+v\"(ai2)); const KhInt4 a2 = p.rec[ai2]; if (a2.w == 0x7ffffff1) c_arc[k].x = a2.x; }\n")
elif name == "dup_store":
    rep("        u.link_k[l] = c_tot[k];\n      });",
        "        u.link_k[l] = c_tot[k];\n        { int l2 = l; asm volatile(\"\" : \"+v\"(l2)); u.link_dst[l2] = -2 - c_arc[k].w; u.link_src[l2] = c_src[k]; u.link_arc[l2] = c_ai[k]; u.link_k[l2] = c_tot[k]; }\n      });")
elif name == "dup_tok":
    rep("    int st = u.tok_state[ic];\n    KH_BOUND(1, st, 0, 0x7ffffff0);",
        "    int st = u.tok_state[ic];\n    { int ic2 = ic; asm volatile(\"\" : \"+v\"(ic2)); const int st2 = u.tok_state[ic2]; const uint32_t co2 = LoadCostEnc(&u.tok_cost[ic2]); if (st2 == 0x7ffffff1 && co2 == 17u) st = 0; }\n    KH_BOUND(1, st, 0, 0x7ffffff0);")
else:
    raise SystemExit("unknown variant " + name)
s = s.replace('#include "kh_common.h"', '#include "/root/repo/old-kaldi-git_amd/csrc/kh_common.h"')
open(b, "w").write(s)
PY
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-result -D__HIP_PLATFORM_AMD__ -mllvm -amdgpu-inline-max-bb=100000 -I$P/csrc -Iinclude -c $src -o /tmp/kh_decoder_$name.o
objs=$(ls $P/build/*.o | grep -v '/kh_decoder\.o$')   # (the host half, build/kh_decoder_host.o, is linked as built: no flags here)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/libkh_exp_$name.so $objs /tmp/kh_decoder_$name.o
echo tools/libkh_exp_$name.so
