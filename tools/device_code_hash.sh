#!/bin/bash
# Hash the device side of scarlet_hip.hip, to show that a host-only change left the code object alone (no GPU needed).
# Compiles the device side for gfx950 with the Makefile's flags, unbundles the ELF, prints the sha256 of .text and
# .rodata and writes the sorted symbol table next to it.   usage: tools/device_code_hash.sh SOURCE_TREE OUT_DIR
# Run it on a checkout of the parent and on the branch, then diff OUT_DIR/symbols.txt of the two: only the
# __hip_cuid_* symbol may differ.
set -e -o pipefail
tree=$(cd "$1" && pwd); mkdir -p "$2"; out=$(cd "$2" && pwd)
llvm=/opt/rocm/lib/llvm/bin
cd "$tree/scarlet_amd/csrc"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include --cuda-device-only -c scarlet_hip.hip \
    -o "$out/device.o" 2>/dev/null
$llvm/clang-offload-bundler --unbundle --type=o --targets=hip-amdgcn-amd-amdhsa--gfx950 --input="$out/device.o" \
    --output="$out/gfx950.elf"
for s in .text .rodata; do
  $llvm/llvm-objcopy -O binary --only-section=$s "$out/gfx950.elf" "$out/section$s.bin"
  echo "$s $(stat -c %s "$out/section$s.bin") bytes sha256 $(sha256sum "$out/section$s.bin" | cut -d' ' -f1)"
done
$llvm/llvm-readelf -sW "$out/gfx950.elf" | awk 'NF >= 8 && $1 ~ /:$/ {print $2, $3, $4, $5, $6, $7, $8}' | sort > "$out/symbols.txt"
echo "$(wc -l < "$out/symbols.txt") symbols -> $out/symbols.txt"
