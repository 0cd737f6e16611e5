"""The record builder and the slab arithmetic of csrc/common.h (rec_build, slab_place, seg_pack) as a stand-alone host program under
AddressSanitizer and UBSan: records cut out of exactly-sized heap buffers against a base-by-base restatement of the format
(tests/host/record_build_main.cpp).  No GPU: the host side of the header is compiled alone."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_builder_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed to compile the host program")
    exe = str(tmp_path / "record_build_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "record_build_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "records equal the base-by-base form" in out.stdout
