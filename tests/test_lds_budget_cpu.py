"""CPU test of the host arithmetic that sizes the probe and count kernels' LDS (charon_amd/csrc/parts/lds_budget.hpp): the
ring-packing rule over every supported (k, window), k1_lds_bytes with and without the offset plane, and the count kernel's derived
budget at the default shape.  The checks themselves are in tools/lds_budget_check.cpp, a stand-alone program built here."""
import os
import subprocess

from tests import util


def test_ring_pack_rule_and_count_budget(tmp_path):
    exe = str(tmp_path / "lds_budget_check")
    src = os.path.join(util.ROOT, "tools", "lds_budget_check.cpp")
    inc = os.path.join(util.ROOT, "charon_amd", "csrc", "parts")
    c = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-I" + inc, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert c.returncode == 0, c.stderr.decode()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    print(p.stdout.decode())
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    assert lines[-1] == "ok" and len(lines) == 3
