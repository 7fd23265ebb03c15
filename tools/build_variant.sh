#!/bin/bash
# A/B builds of the library: tools/build_variant.sh <name> "<extra hipcc flags>"
#   -> adsbdec_amd/lib_var/<name>/libadsbdec_amd.so   (load it with ADSB_LIB_PATH=...)
# Every .hip and .cpp of adsbdec_amd/csrc goes in, by glob: no list here to forget a new unit in.
cd "$(dirname "$0")/.." || exit 1
name=$1; shift
out=adsbdec_amd/lib_var/$name
mkdir -p "$out"
rm -f "$out"/*.o
FLAGS="--offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -Wno-unused-function -mllvm -amdgpu-atomic-optimizer-strategy=None -Xarch_host -mavx2 $*"
for s in adsbdec_amd/csrc/*.hip; do
  /opt/rocm/bin/hipcc $FLAGS -c "$s" -o "$out/$(basename "$s").o" || exit 1
done
gcc -O2 -fPIC -c adsbdec_amd/csrc/format.c -o "$out/format.c.o" || exit 1
for s in adsbdec_amd/csrc/*.cpp; do
  g++ -O2 -fPIC -std=c++17 -pthread -c "$s" -o "$out/$(basename "$s").o" || exit 1
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$out/libadsbdec_amd.so" "$out"/*.o -lm -lpthread || exit 1
echo "$out/libadsbdec_amd.so"
