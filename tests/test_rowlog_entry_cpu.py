"""CPU test of the compact row-log entry and its chain mode (charon_amd/csrc/parts/rowlog_entry.hpp): what k_minimise_probe writes for a
probed row and what k_count_wavelog reads back.  Rows of 0..12 set bins, 1..129 bins, every owner: the entries decode to the row's bin
set, pass A's bumps are its set bits, pass B's found / fbin equal popcount(row & mask) / its bit under 1 000 random chosen-bin masks, a log
cut behind a chain's first entry is walked without a read at or beyond its count, and without chain mode the encoding is bit for bit
what it was.  The checks themselves are in tools/rowlog_entry_check.cpp, a stand-alone program built here with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

from tests import util


def test_entries_chains_and_the_count_kernels_walk(tmp_path):
    exe = str(tmp_path / "rowlog_entry_check")
    src = os.path.join(util.ROOT, "tools", "rowlog_entry_check.cpp")
    inc = os.path.join(util.ROOT, "charon_amd", "csrc", "parts")
    c = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + inc, src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert c.returncode == 0, c.stderr.decode()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    print(p.stdout.decode())
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    assert lines[-1] == "ok" and len(lines) == 2 and " chained " in lines[0]
