"""The absence filter's key (fmer_key of csrc/common.h) per window stride, as a stand-alone host program under AddressSanitizer and
UBSan (tests/host/fmer_runs_main.cpp): the key of a 31-mer equals its reverse complement's (random 31-mers, periods 1, 2, 3, 4, 15, 17
and their complements), the stream bits above 62 are ignored, and the runs of equal words -- the atomics the builder issues -- come in
the order stride 1 < 2 < 4.  No GPU: the host side of the header is compiled alone."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fmer_key_symmetries_and_runs_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed to compile the host program")
    exe = str(tmp_path / "fmer_runs_host")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "fmer_runs_main.cpp"), "-o", exe])
    out = subprocess.run([exe, "300000"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "keys equal their reverse complements' and ignore the bits above 62" in out.stdout
    fig = {int(m.group(1)): {k: int(m.group(i + 2)) for i, k in enumerate(("runs", "cut64", "cut256"))}
           for m in re.finditer(r"stride (\d+): positions \d+ runs (\d+) cut64 (\d+) cut256 (\d+)", out.stdout)}
    assert sorted(fig) == [1, 2, 4]
    for k in ("runs", "cut64", "cut256"):
        assert fig[1][k] < fig[2][k] < fig[4][k], (k, fig)
    # the price of the builder's atomics: all 17 windows at least halve the count of the five-window key, at a wavefront's cut too
    assert 2 * fig[1]["cut64"] <= fig[4]["cut64"], fig
