#!/bin/bash
# Appends the hash of a built library's device code + the compiler to that library's record under tests/golden/ (tests/test_device_hash.py
# pins it): libtrayhip.so -> device_code_hash.txt, libtrayhip_<name>.so -> <name>_device_code_hash.txt. Without a library: libtrayhip.so.
# Run it only after this very build passed `pytest -m gpu` on an MI355X:   tools/record_device_hash.sh "pytest -m gpu 44 passed (...)" [libtrayhip_guide.so]
set -e
cd "$(dirname "$0")/.."
LIB=$(basename "${2:-libtrayhip.so}" .so)
NAME=${LIB#libtrayhip}
RECORD=tests/golden/${NAME:+${NAME#_}_}device_code_hash.txt
[ -f "$RECORD" ] || { echo "no record $RECORD for $LIB.so" >&2; exit 1; }
echo "$(tools/device_code_hash.sh tray_rust_amd/$LIB.so) | $(/opt/rocm/bin/hipcc --version | head -1) | ${1:-GPU run}" >> "$RECORD"
tail -1 "$RECORD"
