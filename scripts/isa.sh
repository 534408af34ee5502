#!/bin/bash
# Device ISA of one kernel source with the library's flags: scripts/isa.sh k_conv.hip [extra flags] -> /tmp/isa/k_conv.s
# The flags are _build's own (COMMON + the source's extra flags + IRMV_EXTRA_HIPCC_FLAGS), as tests/test_isa_lint.py takes them.
set -e
src=$1; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p /tmp/isa
flags=$(cd "$root" && python3 -c "import os, sys; from irmv_detection_amd import _build as b; print(' '.join(b.COMMON + dict(b.SOURCES)[sys.argv[1]] + os.environ.get('IRMV_EXTRA_HIPCC_FLAGS', '').split()))" "$src")
hipcc=$(cd "$root" && python3 -c "from irmv_detection_amd import _build as b; print(b.hipcc())")
out=/tmp/isa/${src%.*}.s
"$hipcc" $flags "$@" --cuda-device-only -S "$root/irmv_detection_amd/csrc/$src" -o "$out"
echo "$out"
