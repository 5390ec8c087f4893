"""GPU test of the prefix sums every kernel shares (charon_amd/csrc/parts/scan.inc): the wave scan, the block step and the
one-workgroup array scan, each compared exactly with a serial loop on the host at the sizes where a lane, a wavefront's partial, a
round of 1024 values or the carry between rounds can go wrong.  The checks themselves are in tools/scan_check.hip, a stand-alone
program built here with the library's flags (csrc/Makefile, without -shared -fPIC) and run once as a child process."""
import os
import subprocess

import pytest

from tests import util


@pytest.mark.gpu
def test_wave_block_and_array_scans(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "scan_check")
    src = os.path.join(util.ROOT, "tools", "scan_check.hip")
    c = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++14", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
                        "-I" + os.path.join(util.ROOT, "include"), "-I" + os.path.join(util.ROOT, "charon_amd", "csrc"), src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert c.returncode == 0, c.stderr.decode()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    print(p.stdout.decode())
    assert p.returncode == 0, p.stdout.decode()[-2000:] + p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    # 15 block-step cases, 10 array cases at each of 14 sizes, 12 with the size read from the device
    assert lines[-1] == "ok" and lines[-2] == "scan_check: 167 cases" and len(lines) == 169
