"""tests/test_device_hash.py for libtrayhip_foldmis.so, the add-on library of the lean tile kernel's folding instantiations (csrc/hip/kernel_fold.h):
its gfx950 code objects are the ones that were last checked on a GPU (tools/device_code_hash.sh against the last line of
tests/golden/foldmis_device_code_hash.txt); a deliberate change of what it compiles -- or of the device headers behind kernels.hip -- comes with a
GPU run and a new line in that record (tools/record_device_hash.sh "<what ran>" libtrayhip_foldmis.so). A hash is tied to the compiler that
produced it: with another hipcc the test only says so."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM, RECORD = "libtrayhip_foldmis", "foldmis_device_code_hash.txt"


def test_device_code_is_the_gpu_checked_one(built):
    objcopy, hipcc = "/opt/rocm/lib/llvm/bin/llvm-objcopy", "/opt/rocm/bin/hipcc"
    if not os.path.exists(objcopy) or not os.path.exists(hipcc):
        pytest.skip("no llvm-objcopy / hipcc in this image")
    last = [l.strip() for l in open(os.path.join(ROOT, "tests", "golden", RECORD)) if l.strip() and not l.startswith("#")][-1]
    want, compiler = [x.strip() for x in last.split("|")][:2]
    have = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0].strip()
    if have != compiler:
        pytest.skip(f"the recorded hash belongs to '{compiler}', this image has '{have}': re-record it from a GPU run")
    lib = os.path.join(ROOT, "tray_rust_amd", STEM + ".so")
    got = subprocess.run([os.path.join(ROOT, "tools", "device_code_hash.sh"), lib], capture_output=True, text=True, check=True).stdout.strip()
    assert got == want, (f"the gfx950 code objects of {STEM}.so changed: run pytest -m gpu on an MI355X, "
                         f"then tools/record_device_hash.sh '<what ran>' {STEM}.so")
