#!/bin/bash
# development build of libamplihip.so with extra -D flags into amplipy_amd/build/libamplihip_dev.so (use: AMPLIHIP_LIB=amplipy_amd/build/libamplihip_dev.so)
# The read pass and the C ABI beside it see the same flags (-DAMP_DEV changes amp_ctx, which both know); the other units of
# the library come from amplipy_amd/build as they are (python -m amplipy_amd.build makes them).
set -e
cd "$(dirname "$0")/.."
mkdir -p amplipy_amd/build
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function"
for u in amp_readpass amplihip; do
  /opt/rocm/bin/hipcc $F "$@" -c -o amplipy_amd/build/${u}_dev.o amplipy_amd/csrc/$u.hip > /tmp/build_dev_$u.log 2>&1 || { grep -B2 -A8 "error" /tmp/build_dev_$u.log | head -60; echo BUILD FAILED; exit 1; }
done
OTHERS=$(for u in amp_ins amp_deflate amp_sam amp_bgzf amp_qc amp_strand amp_amplicon; do echo amplipy_amd/build/$u.o; done)
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o amplipy_amd/build/libamplihip_dev.so amplipy_amd/build/amplihip_dev.o amplipy_amd/build/amp_readpass_dev.o $OTHERS -ldl
echo DEV BUILD OK
