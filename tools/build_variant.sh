#!/bin/bash
# usage: tools/build_variant.sh NAME [-DFLAG ...]  -> tools/libkh_exp_NAME.so (both decoder files rebuilt with the flags)
set -e
cd "$(dirname "$0")/.."
name=$1; shift
P=old-kaldi-git_amd
B="import importlib; b = importlib.import_module('$P.build')"
python -c "$B; b.build()" >/dev/null
# each half with the library's own flags for that file (build.py: FLAGS + EXTRA) and the -D flags of the command line: KH_NT,
# KH_NPH, KH_SERVE_MARKERS, KH_BOUNDS_CHECK and KH_BARRIER_CHECK matter to the kernels (kh_decoder.hip) AND to the host
# code that sizes buffers from them and reads the debug symbols (kh_decoder_host.hip)
for f in kh_decoder kh_decoder_host; do
  /opt/rocm/bin/hipcc $(python -c "$B; print(' '.join(b.flags_for('$f.hip')))") "$@" -c $P/csrc/$f.hip -o /tmp/${f}_$name.o
done
objs=$(ls $P/build/*.o | grep -v -e '/kh_decoder\.o$' -e '/kh_decoder_host\.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/libkh_exp_$name.so $objs /tmp/kh_decoder_$name.o /tmp/kh_decoder_host_$name.o
echo tools/libkh_exp_$name.so
