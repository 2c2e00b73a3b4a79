"""The kernels of the filtered stopping rule (libtrayhip_guide.so, csrc/hip/guide.hip) are the device code last checked on a GPU, as
tests/test_denoise_device_hash.py asks of libtrayhip_denoise.so: a change of their gfx950 code objects comes with a GPU run and a new line in
tests/golden/guide_device_code_hash.txt."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_guide_device_code_is_the_gpu_checked_one(built):
    objcopy, hipcc = "/opt/rocm/lib/llvm/bin/llvm-objcopy", "/opt/rocm/bin/hipcc"
    if not os.path.exists(objcopy) or not os.path.exists(hipcc):
        pytest.skip("no llvm-objcopy / hipcc in this image")
    last = [l.strip() for l in open(os.path.join(ROOT, "tests", "golden", "guide_device_code_hash.txt")) if l.strip() and not l.startswith("#")][-1]
    want, compiler = [x.strip() for x in last.split("|")][:2]
    have = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0].strip()
    if have != compiler:
        pytest.skip(f"the recorded hash belongs to '{compiler}', this image has '{have}': re-record it from a GPU run")
    lib = os.path.join(ROOT, "tray_rust_amd", "libtrayhip_guide.so")
    got = subprocess.run([os.path.join(ROOT, "tools", "device_code_hash.sh"), lib], capture_output=True, text=True, check=True).stdout.strip()
    assert got == want, "the gfx950 code objects of libtrayhip_guide.so changed: run pytest -m gpu on an MI355X, then record the new hash"
