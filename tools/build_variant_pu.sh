#!/bin/bash
# usage: tools/build_variant_pu.sh NAME PU [-DFLAG ...]  -> tools/libkh_exp_NAME.so, the decoder's kernels built from a copy of
# csrc/kh_decoder.hip with `constexpr int PU` set to PU (the source itself, and with it the hash the PMC record carries, stays)
set -e
cd "$(dirname "$0")/.."
name=$1; pu=$2; shift; shift
P=old-kaldi-git_amd
B="import importlib; b = importlib.import_module('$P.build')"
python -c "$B; b.build()" >/dev/null
grep -q '^constexpr int PU = [0-9]*;' $P/csrc/kh_decoder.hip || { echo "build_variant_pu: no 'constexpr int PU' line in kh_decoder.hip" >&2; exit 1; }
sed "s/^constexpr int PU = [0-9]*;/constexpr int PU = $pu;/" $P/csrc/kh_decoder.hip > /tmp/kh_decoder_$name.hip
# the library's own flags for each file (build.py: FLAGS + EXTRA; the device file's include the per-file one); the host half
# of the decoder sees the same -D flags: see build_variant.sh
/opt/rocm/bin/hipcc $(python -c "$B; print(' '.join(b.flags_for('kh_decoder.hip')))") -I$P/csrc -Iinclude "$@" -c -x hip /tmp/kh_decoder_$name.hip -o /tmp/kh_decoder_$name.o
/opt/rocm/bin/hipcc $(python -c "$B; print(' '.join(b.flags_for('kh_decoder_host.hip')))") "$@" -c $P/csrc/kh_decoder_host.hip -o /tmp/kh_decoder_host_$name.o
objs=$(ls $P/build/*.o | grep -v -e '/kh_decoder\.o$' -e '/kh_decoder_host\.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/libkh_exp_$name.so $objs /tmp/kh_decoder_$name.o /tmp/kh_decoder_host_$name.o
echo tools/libkh_exp_$name.so
