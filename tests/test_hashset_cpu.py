"""CPU tests of the device-resident minimiser sets (chn_hashset): the refusals that need no device, the sort's geometry
(charon_amd/csrc/parts/radix_plan.hpp, checked by tools/radix_plan_check.cpp, a stand-alone program built here), and the refusal of
CHARON_GPU_INDEX_SETS values other than 0 and 1 before `charon index` reads its table."""
import ctypes as C
import os
import subprocess

from tests import util

EXE = os.path.join(util.ROOT, "charon_amd", "bin", "charon")


def test_refusals_that_need_no_device():
    import charon_amd.api as api
    L = api.lib()
    out, n, m = C.c_void_p(), C.c_uint64(7), C.c_uint64(7)
    good = api.HashSetCfg(C.sizeof(api.HashSetCfg), 0, 0, 0)
    assert L.chn_hashset_create(None, C.byref(out)) == api.E_INVALID
    assert L.chn_hashset_create(C.byref(good), None) == api.E_INVALID
    for cfg in (api.HashSetCfg(C.sizeof(api.HashSetCfg) - 4, 0, 0, 0), api.HashSetCfg(0, 0, 0, 0),
                api.HashSetCfg(C.sizeof(api.HashSetCfg), 0, 100, 0), api.HashSetCfg(C.sizeof(api.HashSetCfg), 0, 257, 0),
                api.HashSetCfg(C.sizeof(api.HashSetCfg), 0, 4096 + 128, 0), api.HashSetCfg(C.sizeof(api.HashSetCfg), 0, 65536 + 256, 0),
                api.HashSetCfg(C.sizeof(api.HashSetCfg), 0, 0, 1)):
        out.value = 1234
        assert L.chn_hashset_create(C.byref(cfg), C.byref(out)) == api.E_INVALID, (cfg.struct_size, cfg.tile_keys, cfg.reserved)
        assert out.value is None  # no handle where the call fails
    assert b"tile_keys" in L.chn_last_error() or b"reserved" in L.chn_last_error()
    buf = (C.c_uint64 * 4)(1, 2, 3, 4)
    assert L.chn_hashset_append(None, buf, 4) == api.E_INVALID
    assert L.chn_hashset_unique(None, C.byref(n)) == api.E_INVALID
    assert L.chn_hashset_size(None, C.byref(n), C.byref(m)) == api.E_INVALID
    assert L.chn_hashset_download(None, 0, 4, buf) == api.E_INVALID
    assert list(buf) == [1, 2, 3, 4] and (n.value, m.value) == (7, 7)
    batch = api.Batch()
    assert L.chn_minimisers_into(None, C.byref(batch), None, C.byref(n)) == api.E_INVALID
    assert L.chn_index_emplace_set(None, None, 0) == api.E_INVALID
    assert L.chn_device_memory(0, None, None) == api.E_INVALID
    assert L.chn_hashset_destroy(None) == 0


def test_radix_plan(tmp_path):
    exe = str(tmp_path / "radix_plan_check")
    src = os.path.join(util.ROOT, "tools", "radix_plan_check.cpp")
    inc = os.path.join(util.ROOT, "charon_amd", "csrc", "parts")
    c = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-I" + inc, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert c.returncode == 0, c.stderr.decode()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    print(p.stdout.decode())
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    assert lines[-1] == "ok" and len(lines) == 10
    assert lines[0] == "n 0 tile 4096: 0 tiles, 0 bytes of scratch"
    assert lines[5].startswith("n 4294967295 tile 4096: 1048576 tiles, ")


def test_other_values_of_the_switch_end_the_run_before_the_table_is_read(tmp_path):
    tab = tmp_path / "in.tab"
    tab.write_text("%s\tmicrobial\n" % (tmp_path / "no_such_file.fa"))
    log = tmp_path / "two.log"
    env = {k: v for k, v in os.environ.items() if not k.startswith("CHARON_")}
    env["CHARON_GPU_INDEX_SETS"] = "2"
    p = subprocess.run([EXE, "index", "-p", str(tmp_path / "two"), "--log", str(log), str(tab)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    err = p.stderr.decode()
    assert p.returncode == 1 and "CHARON_GPU_INDEX_SETS" in err and "neither 0 nor 1" in err, err
    assert not (tmp_path / "two.idx").exists()
    assert "Found " not in (log.read_text() if log.exists() else "")
