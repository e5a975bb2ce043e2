#!/bin/bash
# development build with extra -D flags into amplipy_amd/build/dev_<tag>.so: tools/bdev_tag.sh <tag> -DX=1 ...
# (the read pass and the C ABI beside it see the same flags; the other units come from amplipy_amd/build as they are)
set -e
cd "$(dirname "$0")/.."
tag=$1; shift
mkdir -p amplipy_amd/build
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function"
for u in amp_readpass amplihip; do
  /opt/rocm/bin/hipcc $F "$@" -c -o amplipy_amd/build/dev_${tag}_$u.o amplipy_amd/csrc/$u.hip > /tmp/build_dev_${tag}_$u.log 2>&1 || { grep -B2 -A8 "error" /tmp/build_dev_${tag}_$u.log | head -60; echo BUILD FAILED; exit 1; }
done
OTHERS=$(for u in amp_ins amp_deflate amp_sam amp_bgzf amp_qc amp_strand amp_amplicon; do echo amplipy_amd/build/$u.o; done)
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o amplipy_amd/build/dev_$tag.so amplipy_amd/build/dev_${tag}_amplihip.o amplipy_amd/build/dev_${tag}_amp_readpass.o $OTHERS -ldl
rm -f amplipy_amd/build/dev_${tag}_amplihip.o amplipy_amd/build/dev_${tag}_amp_readpass.o
echo DEV BUILD $tag OK
