#!/bin/bash
# usage: tools/kernel_resources.sh [-DFLAG ...]   compile-only check of the decoder kernels' registers / scratch
# (-Rpass-analysis=kernel-resource-usage; no GPU needed).  ScratchSize of DecodeKernel<1,0> is what to watch.
cd "$(dirname "$0")/.."
mkdir -p old-kaldi-git_amd/build/kernel_resources   # (under the package's ignored build directory, not a fixed name in a directory users share; a subdirectory: the variant scripts link build/*.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-result -D__HIP_PLATFORM_AMD__ \
  -mllvm -amdgpu-inline-max-bb=100000 -mllvm -disable-machine-licm -Rpass-analysis=kernel-resource-usage "$@" -c old-kaldi-git_amd/csrc/kh_decoder.hip -o old-kaldi-git_amd/build/kernel_resources/kh_decoder.o 2>&1 |
  awk '/Function Name/ {n=$0; sub(/.*Name: /,"",n); sub(/ \[.*/,"",n)} /VGPRs:/ {v=$0; sub(/.*VGPRs: /,"",v); sub(/ \[.*/,"",v)} /ScratchSize/ {s=$0; sub(/.*: /,"",s); sub(/ \[.*/,"",s); } /Occupancy/ {print substr(n,1,60), "VGPRs", v, "Scratch", s}'
