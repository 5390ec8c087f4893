#!/usr/bin/env python3
"""Measurements of BGZF members inflated on the device (chn_inflate_run[_crc] / k_inflate_members, CHARON_GPU_INFLATE=1).  Needs an MI355X.

usage: python tools/gpu_inflate_bench.py [n_reads] [workdir] [rounds] [threads ...]
The workload of tools/cli_steady_state.py (5 kb reads from two 2 Mb genomes, index by this build's `charon index`), written as BGZF with
tools/make_bgzf.py.
  1. api.Inflater.run_job alone on the file's first 64, 1 024 and 4 096 members: GB/s of text for the whole call (pack + upload + decode +
     download) with input and output in page-locked and in pageable memory, and the kernels' own time from events (chn_inflate_kernel_ms);
     the same with the CRC-32 taken and compared on the device (chn_inflate_run_crc with the trailers' values), alternated with the
     plain call; chn_inflate_run_host on one thread and Python's zlib beside it; and the pass the device CRC replaces -- fast_crc32
     over the same members on the reader's threads at every -t (`charon _bgzf_crc`).
  2. `charon dehost` on the BGZF file for every round, every -t and every configuration in turn: PARENT_CHARON=<the parent commit's
     charon> (if set) with the switch unset and with CHARON_GPU_INFLATE=1, this build with the switch unset, this build with CHARON_GPU_INFLATE=1.  Wall time, reads/s, the reader's timers
     (CHARON_TIMING) with the reader's `inflate` beside `inside chn_inflate_run` and their difference (what the reader does around
     the call: member list, descriptors and, before the device CRC, the CRC pass), min - max per configuration, and whether every run
     wrote the same TSV (sha256).
Everything is printed; nothing is asserted."""
import ctypes as C
import hashlib
import importlib.util
import os
import re
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return sorted(v)[len(v) // 2]


def bgzf_members(path, limit):
    """(deflate data, inflated size, CRC-32 of the trailer) of the first `limit` non-empty members of a BGZF file"""
    out = []
    with open(path, "rb") as f:
        while len(out) < limit:
            head = f.read(18)
            if len(head) < 18:
                break
            assert head[:4] == b"\x1f\x8b\x08\x04" and head[12:14] == b"BC"
            total = struct.unpack("<H", head[16:18])[0] + 1
            body = f.read(total - 18)
            isize = struct.unpack("<I", body[-4:])[0]
            if isize:
                out.append((body[:-8], isize, struct.unpack("<I", body[-8:-4])[0]))
    return out


def api_part(bgzf, exe, threads, reps=7):
    import charon_amd.api as api
    every = bgzf_members(bgzf, 4096)
    h = api.Inflater(0)
    for n in (64, 1024, 4096):
        ms = every[:n]
        if len(ms) < n:
            print("only %d members in the file: job of %d skipped" % (len(ms), n))
            continue
        members, sizes, crcs = [m for m, _, _ in ms], [s for _, s, _ in ms], [c for _, _, c in ms]
        text = sum(sizes)
        comp = sum(len(m) for m in members)
        for kind in ("pageable", "page-locked"):
            j, a = api.inflate_job(members, sizes)
            keep = []
            if kind == "page-locked":
                pin_in = api.pinned_array(a["data"].size, np.uint8)
                pin_in[:] = a["data"]
                pin_out = api.pinned_array(text, np.uint8)
                j.in_, j.out = pin_in.ctypes.data, pin_out.ctypes.data
                keep = [pin_in, pin_out]
                a["out"] = pin_out
            c, ca = api.inflate_crc(n, crcs, True)
            wall, kern, wall_c, kern_c = [], [], [], []
            for i in range(reps + 1):  # plain and with CRC in turn
                t0 = time.perf_counter()
                h.run_job(j)
                dt = time.perf_counter() - t0
                if i:  # the first call allocates
                    wall.append(dt)
                    kern.append(h.kernel_ms() / 1e3)
                assert not a["status"][:n].any()
                t0 = time.perf_counter()
                h.run_job(j, c)
                dt = time.perf_counter() - t0
                if i:
                    wall_c.append(dt)
                    kern_c.append(h.kernel_ms() / 1e3)
                assert not a["status"][:n].any() and (ca["crc32"][:n] == np.array(crcs, np.uint32)).all()
            at = int(a["out_offset"][n - 1])
            assert a["out"][at:at + sizes[-1]].tobytes() == zlib.decompressobj(-15).decompress(members[-1])
            print("chn_inflate_run %5d members, %6.1f MB of text (%5.1f MB deflated), %-11s: call min %.2f median %.2f max %.2f ms -> %.2f GB/s of text (median); "
                  "kernels median %.2f ms -> %.2f GB/s" % (n, text / 1e6, comp / 1e6, kind, min(wall) * 1e3, med(wall) * 1e3, max(wall) * 1e3, text / med(wall) / 1e9,
                                                           med(kern) * 1e3, text / med(kern) / 1e9), flush=True)
            print("   with CRC (chn_inflate_run_crc)%*s: call min %.2f median %.2f max %.2f ms -> %.2f GB/s of text (median); kernels min %.2f median %.2f max %.2f ms -> %.2f GB/s"
                  "   [plain kernels min %.2f max %.2f ms; CRC adds %+.2f ms to the median, %+.1f %%]"
                  % (len(kind) + 21, kind, min(wall_c) * 1e3, med(wall_c) * 1e3, max(wall_c) * 1e3, text / med(wall_c) / 1e9, min(kern_c) * 1e3, med(kern_c) * 1e3,
                     max(kern_c) * 1e3, text / med(kern_c) / 1e9, min(kern) * 1e3, max(kern) * 1e3, (med(kern_c) - med(kern)) * 1e3,
                     100 * (med(kern_c) - med(kern)) / med(kern)), flush=True)
            for p in keep:
                api.host_free(p)
        j, a = api.inflate_job(members, sizes)
        t0 = time.perf_counter()
        api._chk(api.lib().chn_inflate_run_host(C.byref(j)))
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        for m in members:
            zlib.decompressobj(-15).decompress(m)
        t_z = time.perf_counter() - t0
        print("   the same members on one CPU thread: chn_inflate_run_host %.2f GB/s, Python's zlib %.2f GB/s" % (text / t_host / 1e9, text / t_z / 1e9), flush=True)
        for t in threads:  # the pass CHARON_GPU_INFLATE=1 used to run behind the call
            p = subprocess.run([exe, "_bgzf_crc", bgzf, str(n), str(t), str(reps)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            print("   host fast_crc32 pass at -t %2d: %s" % (t, (p.stdout.decode().strip() or p.stderr.decode().strip())), flush=True)
    h.destroy()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
    work = sys.argv[2] if len(sys.argv) > 2 else "/tmp/charon_gpu_inflate"
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    threads = [int(x) for x in sys.argv[4:]] or [1, 16]
    spec = importlib.util.spec_from_file_location("cli_steady_state", os.path.join(ROOT, "tools", "cli_steady_state.py"))
    css = importlib.util.module_from_spec(spec)
    sys.modules["cli_steady_state"] = css  # (its pool of writers pickles the module's block function by name)
    spec.loader.exec_module(css)
    os.makedirs(work, exist_ok=True)
    from tests import util
    r = util.rng(1)
    gs = [util.random_seq(r, 2_000_000), util.random_seq(r, 2_000_000)]
    exe = os.path.join(ROOT, "charon_amd", "bin", "charon")
    with open(os.path.join(work, "refs.tsv"), "w") as tab:
        for name, g in (("microbial", gs[0]), ("human", gs[1])):
            fa = os.path.join(work, name + ".fa")
            with open(fa, "wb") as f:
                f.write(b">" + name.encode() + b"\n" + g + b"\n")
            tab.write("%s\t%s\n" % (fa, name))
    if os.path.exists(os.path.join(work, "bench.idx")):
        os.remove(os.path.join(work, "bench.idx"))
    p = subprocess.run([exe, "index", "-p", os.path.join(work, "bench"), "--log", os.path.join(work, "i.log"), os.path.join(work, "refs.tsv")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode:
        sys.exit("charon index failed: " + p.stderr.decode()[-500:])
    fq, bgzf = os.path.join(work, "reads.fastq"), os.path.join(work, "reads.fastq.gz")
    t0 = time.time()
    css.write_fastq(fq, n, gs)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_bgzf.py"), fq, bgzf, "6", "16"], check=True)
    print("fastq: %d reads of %d bases, %.2f GB of text, %.2f GB as BGZF, written in %.0f s" % (n, css.L, os.path.getsize(fq) / 1e9, os.path.getsize(bgzf) / 1e9, time.time() - t0),
          flush=True)
    os.remove(fq)
    api_part(bgzf, exe, threads)

    parent = os.environ.get("PARENT_CHARON")
    configs = (([("parent", parent, {}), ("parent GPU_INFLATE=1", parent, {"CHARON_GPU_INFLATE": "1"})] if parent else []) +
               [("unset", exe, {}), ("CHARON_GPU_INFLATE=1", exe, {"CHARON_GPU_INFLATE": "1"})])
    digests, rates, around = set(), {}, {}
    for rnd in range(rounds):
        for t in threads:
            for name, binary, extra in configs:
                env = {k: v for k, v in os.environ.items() if k != "CHARON_GPU_INFLATE"}
                env["CHARON_TIMING"] = "1"
                env.update(extra)
                out = os.path.join(work, "out.tsv")
                t0 = time.time()
                with open(out, "wb") as fo:
                    p = subprocess.run([binary, "dehost", "--db", os.path.join(work, "bench.idx"), "-t", str(t), "--log", os.path.join(work, "c.log"), bgzf],
                                       stdout=fo, stderr=subprocess.PIPE, env=env, timeout=600)
                dt = time.time() - t0
                hsh = hashlib.sha256()
                with open(out, "rb") as fi:
                    for chunk in iter(lambda: fi.read(1 << 24), b""):
                        hsh.update(chunk)
                os.remove(out)
                digests.add(hsh.hexdigest())
                rates.setdefault((name, t), []).append(n / dt)
                print("round %d %-20s -t %2d: rc=%d wall %.2f s -> %.0f reads/s   tsv sha256 %s" % (rnd, name, t, p.returncode, dt, n / dt, hsh.hexdigest()[:16]), flush=True)
                err = p.stderr.decode()
                for line in err.splitlines():
                    if "timing (reader" in line or "timing (main" in line:
                        print("   " + line.strip(), flush=True)
                fill, inside = re.search(r"reader thread, s\): inflate ([0-9.]+)", err), re.search(r"inside chn_inflate_run ([0-9.]+)", err)
                if fill and inside:
                    d = float(fill.group(1)) - float(inside.group(1))
                    around.setdefault((name, t), []).append(d)
                    print("   reader inflate %.3f s, inside chn_inflate_run %.3f s, around the call %.3f s" % (float(fill.group(1)), float(inside.group(1)), d), flush=True)
                if p.returncode:
                    sys.exit("charon dehost failed: " + p.stderr.decode()[-800:])
    for (name, t), v in sorted(rates.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print("%-20s -t %2d: min %.0f  median %.0f  max %.0f reads/s over %d runs" % (name, t, min(v), med(v), max(v), len(v)))
    for (name, t), v in sorted(around.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print("%-20s -t %2d: reader inflate minus inside chn_inflate_run: min %.3f  median %.3f  max %.3f s over %d runs" % (name, t, min(v), med(v), max(v), len(v)))
    print("TSV identical across runs: %s" % (len(digests) == 1))


if __name__ == "__main__":
    main()
