"""CPU test of the host arithmetic of a batch's chain (charon_amd/csrc/parts/batch_plan.inc): the gzip column's plan (occupancy classes,
the long-read list longest first, the handed-back list) against a brute-force restatement, the layout of a slot's result block, the
dispatch on bin_words, the numbers of chn_stream_profile, waves_of and split_bound.  The checks themselves are in
tools/stream_batch_check.hip, a stand-alone program that makes no HIP call, built here with the address and undefined-behaviour
sanitizers on the host side."""
import os
import subprocess

from tests import util


def test_gzip_plan_result_layout_and_dispatch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "stream_batch_check")
    src = os.path.join(util.ROOT, "tools", "stream_batch_check.hip")
    c = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++14", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(util.ROOT, "include"),
                        "-I" + os.path.join(util.ROOT, "charon_amd", "csrc"), src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert c.returncode == 0, c.stderr.decode()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    print(p.stdout.decode())
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    assert lines[-1] == "ok" and len(lines) == 2 and lines[0].startswith("stream_batch_check: 60 gzip plans; ")
