"""CPU test of the thread machinery of `charon dehost` (charon_amd/csrc/host/flight_pool.inc, row_writer.inc, replica_set.inc over
ordered_merge.inc) with stub flights and stub callables: 1, 2, 3 and 8 replicas with 0 to 300 flights reach the writer exactly once and
in input order, never more than kMaxOutstanding per replica nor more than two queued at the writer; hand-over switched off and on
again in the middle; a submit, a wait and a row callable that throw at the first, a middle and the last flight surface once on the
main thread with the message the command line gives, every thread joined and every flight freed; the pool hands back the same
objects.  The checks themselves are in tools/dehost_pipeline_check.cpp, a stand-alone program built here twice: with the thread
sanitizer, and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from tests import util


@pytest.mark.parametrize("sanitizers", [["-fsanitize=thread"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["thread", "address-undefined"])
def test_writer_replicas_and_pool_under_sanitizers(tmp_path, sanitizers):
    exe = str(tmp_path / "dehost_pipeline_check")
    src = os.path.join(util.ROOT, "tools", "dehost_pipeline_check.cpp")
    inc = os.path.join(util.ROOT, "charon_amd", "csrc", "host")
    c = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-pthread"] + sanitizers + ["-I" + inc, src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert c.returncode == 0, c.stderr.decode()
    assert b"warning" not in c.stderr, c.stderr.decode()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    print(p.stdout.decode())
    assert p.returncode == 0, p.stderr.decode()
    assert p.stderr == b"", p.stderr.decode()  # (a sanitizer report that did not end the run)
    lines = p.stdout.decode().splitlines()
    assert lines[-1] == "ok" and len(lines) == 2 and lines[0].startswith("flights made and freed: ")
