#!/usr/bin/env python3
"""Measurements of extract files deflated on the device (chn_deflate_run / k_deflate_members, CHARON_GPU_DEFLATE=1).  Needs an MI355X.

usage: python tools/gpu_deflate_bench.py [n_reads] [workdir] [rounds] [threads ...]      (n_reads 0: part 1 only)
  1. api.Deflater.run_job alone on 64, 1 024 and 4 096 pieces of 65 280 bytes of the 5 kb FASTQ fixture of tests/deflate_cases.py, as
     BGZF: GB/s of text for the whole call (pack + upload + compress + gather + download) with input and output in pageable and in
     page-locked memory, the kernels' own time from events (chn_deflate_kernel_ms), the size against zlib level 1 and 6;
     chn_deflate_run_host and Python's zlib level 6 on one thread beside it (on the first 64 pieces).
  2. `charon dehost --extract all` on the workload of tools/cli_steady_state.py (5 kb reads from two 2 Mb genomes, index by this build's
     `charon index`: nearly every read is called) for every round, every -t and every configuration in turn: PARENT_CHARON=<the parent
     commit's charon> (if set), this build with the switch unset, this build with CHARON_GPU_DEFLATE=1.  Wall time, reads/s,
     `inside chn_deflate_run` (CHARON_TIMING) and its share, min - max per configuration, the extract files' sizes, and whether every
     run wrote the same TSV and the same extracted text (sha256 of the decompressed files).
Everything is printed; nothing is asserted beyond the round trip of part 1."""
import ctypes as C
import gzip
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return sorted(v)[len(v) // 2]


def api_part(reps=5):
    import charon_amd.api as api
    from tests import deflate_cases as dc
    t0 = time.time()
    text = dc.fastq_5kb(4096 * dc.MAX_IN, 31)
    every = dc.pieces_of(text)
    print("fixture: %.1f MB of 5 kb reads in %.0f s" % (len(text) / 1e6, time.time() - t0), flush=True)
    h = api.Deflater(0)
    flags = api.DEFLATE_BGZF
    for n in (64, 1024, 4096):
        total = n * dc.MAX_IN
        where = [(i * dc.MAX_IN, dc.MAX_IN) for i in range(n)]
        for kind in ("pageable", "page-locked"):
            bound = api.deflate_bound(n, total, flags)
            if kind == "page-locked":
                data, out = api.pinned_array(total, np.uint8), api.pinned_array(bound, np.uint8)
                data[:] = np.frombuffer(text[:total], np.uint8)
            else:
                data, out = np.frombuffer(text[:total], np.uint8), np.empty(bound, np.uint8)
            j, a = api.deflate_job(where, flags, data=data, out=out)
            wall, kern = [], []
            for i in range(reps + 1):
                t0 = time.perf_counter()
                h.run_job(j)
                dt = time.perf_counter() - t0
                if i:  # the first call allocates
                    wall.append(dt)
                    kern.append(h.kernel_ms() / 1e3)
            used = int(a["used"][0])
            if kind == "pageable":
                assert gzip.decompress(out[:used].tobytes()) == text[:total]
            print("chn_deflate_run %5d pieces, %6.1f MB of text -> %6.1f MB, %-11s: call min %.2f median %.2f max %.2f ms -> %.2f GB/s of text (median); "
                  "kernels min %.2f median %.2f max %.2f ms -> %.2f GB/s" % (n, total / 1e6, used / 1e6, kind, min(wall) * 1e3, med(wall) * 1e3, max(wall) * 1e3,
                                                                             total / med(wall) / 1e9, min(kern) * 1e3, med(kern) * 1e3, max(kern) * 1e3, total / med(kern) / 1e9), flush=True)
            if kind == "page-locked":
                api.host_free(data)
                api.host_free(out)
    first = every[:64]
    j, a = api.deflate_job(first, flags)
    t0 = time.perf_counter()
    api._chk(api.lib().chn_deflate_run_host(C.byref(j)))
    t_host = time.perf_counter() - t0
    sizes = {}
    for level in (1, 6):
        t0 = time.perf_counter()
        sizes[level] = dc.zlib_raw_total(first, level)
        if level == 6:
            t_z = time.perf_counter() - t0
    n_text = sum(map(len, first))
    ours = int(a["used"][0]) - 26 * 64
    print("   64 pieces on one CPU thread: chn_deflate_run_host %.1f MB/s, Python's zlib level 6 %.1f MB/s; raw deflate bytes: ours %d, zlib 1 %d, zlib 6 %d (%.3f / %.3f)"
          % (n_text / t_host / 1e6, n_text / t_z / 1e6, ours, sizes[1], sizes[6], ours / sizes[1], ours / sizes[6]), flush=True)
    h.destroy()


def sha_of(path, unzip):
    hsh = hashlib.sha256()
    with (gzip.open(path, "rb") if unzip else open(path, "rb")) as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            hsh.update(chunk)
    return hsh.hexdigest()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
    work = sys.argv[2] if len(sys.argv) > 2 else "/tmp/charon_gpu_deflate"
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    threads = [int(x) for x in sys.argv[4:]] or [1, 16]
    api_part()
    if n == 0:
        return
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
    fq = os.path.join(work, "reads.fastq")
    t0 = time.time()
    css.write_fastq(fq, n, gs)
    print("fastq: %d reads of %d bases, %.2f GB of text, written in %.0f s" % (n, css.L, os.path.getsize(fq) / 1e9, time.time() - t0), flush=True)

    parent = os.environ.get("PARENT_CHARON")
    configs = ([("parent", parent, {})] if parent else []) + [("unset", exe, {}), ("CHARON_GPU_DEFLATE=1", exe, {"CHARON_GPU_DEFLATE": "1"})]
    tsvs, texts, rates, shares = set(), set(), {}, {}
    for rnd in range(rounds):
        for t in threads:
            for name, binary, extra in configs:
                env = {k: v for k, v in os.environ.items() if k != "CHARON_GPU_DEFLATE"}
                env["CHARON_TIMING"] = "1"
                env.update(extra)
                out, pre = os.path.join(work, "out.tsv"), os.path.join(work, "x")
                t0 = time.time()
                with open(out, "wb") as fo:
                    p = subprocess.run([binary, "dehost", "--db", os.path.join(work, "bench.idx"), "-t", str(t), "--extract", "all", "-p", pre,
                                        "--log", os.path.join(work, "c.log"), fq], stdout=fo, stderr=subprocess.PIPE, env=env, timeout=1100)
                dt = time.time() - t0
                err = p.stderr.decode()
                if p.returncode:
                    sys.exit("charon dehost failed: " + err[-800:])
                files = sorted(f for f in os.listdir(work) if f.startswith("x_") and f.endswith(".gz"))
                size = sum(os.path.getsize(os.path.join(work, f)) for f in files)
                tsv = sha_of(out, False)
                tsvs.add(tsv)
                rates.setdefault((name, t), []).append(n / dt)
                inside = re.search(r"inside chn_deflate_run ([0-9.]+)", err)
                note = ""
                if inside:
                    shares.setdefault((name, t), []).append(float(inside.group(1)) / dt)
                    note = "   inside chn_deflate_run %.2f s (%.0f %%)" % (float(inside.group(1)), 100 * float(inside.group(1)) / dt)
                print("round %d %-20s -t %2d: wall %.2f s -> %.0f reads/s   extract files %.1f MB   tsv sha256 %s%s" % (rnd, name, t, dt, n / dt, size / 1e6, tsv[:16], note), flush=True)
                if rnd == 0:  # the extracted text, once per configuration and -t
                    text = " ".join("%s:%s" % (f, sha_of(os.path.join(work, f), True)[:16]) for f in files)
                    texts.add(text)
                    print("   decompressed: " + text, flush=True)
                for f in files:
                    os.remove(os.path.join(work, f))
                os.remove(out)
    for (name, t), v in sorted(rates.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        s = shares.get((name, t))
        print("%-20s -t %2d: min %.0f  median %.0f  max %.0f reads/s over %d runs%s" % (name, t, min(v), med(v), max(v), len(v),
              "   inside chn_deflate_run %.0f - %.0f %% of the wall time" % (100 * min(s), 100 * max(s)) if s else ""))
    print("TSV identical across runs: %s; extracted text identical across configurations: %s" % (len(tsvs) == 1, len(texts) == 1))
    os.remove(fq)


if __name__ == "__main__":
    main()
