#!/usr/bin/env python3
"""Measurements of one-stream .gz inflated on the device (chn_inflate_stream_run: k_inflate_chunks, k_inflate_windows, k_inflate_bytes;
CHARON_GPU_INFLATE=1 CHARON_GPU_INFLATE_STREAM=1).  Needs an MI355X.

usage: python tools/gpu_inflate_stream_bench.py api [n_reads] [reps]
       python tools/gpu_inflate_stream_bench.py cli [n_reads] [workdir] [rounds] [threads ...]
The reads are those of tools/cli_steady_state.py (5 kb reads from two 2 Mb genomes).
  api  n_reads (default 52 000: 64 MiB and more of deflate data) as ONE raw deflate stream, level 6, with a sync flush at 512 evenly
       spaced record ends -- true block starts.  One round over the whole stretch at 128, 256 and 512 chunks (every fourth, every second,
       every flush point), alternating, `reps` times each after a warm-up: the kernels' device time (chn_inflate_kernel_ms) and GB/s of
       text by it, the whole call's wall time (upload, three kernels, download into pageable memory) and with CHN_INFLATE_OUT_DEVICE
       (no download); chn_inflate_stream_run_host on one thread over the first sixteenth, and Python's zlib over the same, beside it.
       Every run's bytes are compared with the text.
  cli  `charon dehost` on the workload as a `gzip -1` file for every round, every -t and every configuration in turn:
       PARENT_CHARON=<the parent commit's charon> (if set), this build with the switches unset, this build with both switches on.  Wall time,
       reads/s, min - median - max per configuration, the reader's timers and four traced device rounds of the first round, and whether every
       run wrote the same TSV.  Which configuration runs first rotates from round to round.
Everything is printed; nothing is asserted but the bytes."""
import hashlib
import importlib.util
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return sorted(v)[len(v) // 2]


def steady():
    spec = importlib.util.spec_from_file_location("cli_steady_state", os.path.join(ROOT, "tools", "cli_steady_state.py"))
    css = importlib.util.module_from_spec(spec)
    sys.modules["cli_steady_state"] = css  # (its pool of writers pickles the module's block function by name)
    spec.loader.exec_module(css)
    return css


def genomes():
    from tests import util
    r = util.rng(1)
    return [util.random_seq(r, 2_000_000), util.random_seq(r, 2_000_000)]


def cmd_api(argv):
    import charon_amd.api as api
    n = int(argv[0]) if argv else 52000
    reps = int(argv[1]) if len(argv) > 1 else 5
    css = steady()
    path = "/tmp/charon_stream_api.fastq"
    css.write_fastq(path, n, genomes())
    text = open(path, "rb").read()
    os.remove(path)
    t0 = time.time()
    points = [css.REC * ((n * k) // 512) for k in range(1, 512)]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts, cuts, at, size = [], [0], 0, 0
    for p in points + [len(text)]:
        b = c.compress(text[at:p]) + (c.flush(zlib.Z_SYNC_FLUSH) if p < len(text) else c.flush())
        parts.append(b)
        size += len(b)
        at = p
        if p < len(text):
            cuts.append(size)
    data = b"".join(parts)
    print("stream: %d reads, %.1f MB of text, %.1f MiB of deflate data (level 6, %d flush points), made in %.0f s" %
          (n, len(text) / 1e6, len(data) / 2 ** 20, len(points), time.time() - t0), flush=True)
    tpoints = [0] + points
    h = api.Inflater(0)
    jobs = {}
    for chunks in (128, 256, 512):
        step = 512 // chunks
        begin = [8 * cuts[i] for i in range(0, 512, step)]
        target = begin[1:] + [8 * len(data)]
        cap = max(api.INFLATE_STREAM_MIN_SYMS, max(b - a for a, b in zip(tpoints[::step], tpoints[step::step] + [len(text)])) + 4096)
        jobs[chunks] = api.inflate_stream_job(data, begin, target, sym_capacity=cap, out_bytes=len(text))
    dev = api.device_malloc(0, len(text) + 64)
    for chunks in (128, 256, 512):  # warm-up, and the check of the bytes
        j, a = jobs[chunks]
        h.run_stream_job(j)
        assert int(a["counts"][0]) == chunks and int(a["counts"][1]) == len(text) and a["out"][:len(text)].tobytes() == text, chunks
    res = {}
    for rep in range(reps):
        for chunks in (128, 256, 512):
            j, a = jobs[chunks]
            t0 = time.perf_counter()
            h.run_stream_job(j)
            wall = time.perf_counter() - t0
            ms = h.kernel_ms()
            out, ob, fl = j.out, j.out_bytes, j.flags
            j.out, j.flags = dev, api.INFLATE_OUT_DEVICE
            t0 = time.perf_counter()
            h.run_stream_job(j)
            wall_dev = time.perf_counter() - t0
            ms_dev = h.kernel_ms()
            j.out, j.flags = out, fl
            assert int(a["counts"][1]) == len(text)
            res.setdefault(chunks, []).append((ms, wall, ms_dev, wall_dev))
            print("rep %d, %3d chunks: kernels %.2f ms (%.2f GB/s of text), call %.1f ms (%.2f GB/s); into device memory: kernels %.2f ms, call %.1f ms (%.2f GB/s)" %
                  (rep, chunks, ms, len(text) / ms / 1e6, wall * 1e3, len(text) / wall / 1e9, ms_dev, wall_dev * 1e3, len(text) / wall_dev / 1e9), flush=True)
    got = api.device_download(0, dev, len(text), np.uint8)
    assert got.tobytes() == text
    api.device_free(0, dev)
    for chunks, v in sorted(res.items()):
        ks = [x[0] for x in v]
        ws = [x[1] for x in v]
        wd = [x[3] for x in v]
        print("%3d chunks: kernels min %.2f median %.2f max %.2f ms -> %.2f GB/s of text (median); call median %.1f ms -> %.2f GB/s; into device memory %.1f ms -> %.2f GB/s" %
              (chunks, min(ks), med(ks), max(ks), len(text) / med(ks) / 1e6, med(ws) * 1e3, len(text) / med(ws) / 1e9, med(wd) * 1e3, len(text) / med(wd) / 1e9))
    h.destroy()
    # the host form and zlib over the first sixteenth (32 flush points)
    end_d, end_t = cuts[32], tpoints[32]
    begin = [8 * cuts[i] for i in range(32)]
    t0 = time.perf_counter()
    r = api.inflate_stream_host(data[:end_d], begin, begin[1:] + [8 * end_d], sym_capacity=max(api.INFLATE_STREAM_MIN_SYMS, end_t // 32 + 65536), out_bytes=end_t)
    t_host = time.perf_counter() - t0
    assert r["bytes"] == text[:end_t]
    t0 = time.perf_counter()
    z = zlib.decompressobj(-15).decompress(data[:end_d])
    t_z = time.perf_counter() - t0
    assert z == text[:end_t]
    print("one CPU thread over %.1f MB of text: chn_inflate_stream_run_host %.2f GB/s, zlib's inflate %.2f GB/s" % (end_t / 1e6, end_t / t_host / 1e9, end_t / t_z / 1e9))


def cmd_cli(argv):
    n = int(argv[0]) if argv else 400000
    work = argv[1] if len(argv) > 1 else "/tmp/charon_stream_cli"
    rounds = int(argv[2]) if len(argv) > 2 else 3
    threads = [int(x) for x in argv[3:]] or [1, 16]
    css = steady()
    os.makedirs(work, exist_ok=True)
    gs = genomes()
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
    gz = os.path.join(work, "one.fastq.gz")
    t0 = time.time()
    css.write_fastq(fq, n, gs)
    subprocess.run("gzip -1 -c %s > %s" % (fq, gz), shell=True, check=True)
    print("input: %d reads of %d bases; plain %.2f GB, one-stream .gz %.2f GB; prepared in %.0f s" % (n, css.L, os.path.getsize(fq) / 1e9, os.path.getsize(gz) / 1e9,
                                                                                                  time.time() - t0), flush=True)
    os.remove(fq)
    parent = os.environ.get("PARENT_CHARON")
    settings = (["parent"] if parent else []) + ["unset", "on"]
    switches = ("CHARON_GPU_INFLATE", "CHARON_GPU_INFLATE_STREAM")
    digests, rates = set(), {}
    for rnd in range(rounds):
        for t in threads:
            for setting in settings[rnd % len(settings):] + settings[:rnd % len(settings)]:  # (whoever runs first rotates)
                env = {k: v for k, v in os.environ.items() if k not in switches}
                env["CHARON_TIMING"] = "1"
                if setting == "on":
                    env.update(CHARON_GPU_INFLATE="1", CHARON_GPU_INFLATE_STREAM="1", CHARON_DIAG_INFLATE="1")
                    if rnd == 0:
                        env["CHARON_DIAG_INFLATE_ROUNDS"] = "1"  # (the first round's runs trace their rounds: they are not the ones to compare)
                out = os.path.join(work, "out.tsv")
                t0 = time.time()
                with open(out, "wb") as fo:
                    p = subprocess.run([parent if setting == "parent" else exe, "dehost", "--db", os.path.join(work, "bench.idx"), "-t", str(t), "--log",
                                        os.path.join(work, "c.log"), gz], stdout=fo, stderr=subprocess.PIPE, env=env, timeout=900)
                dt = time.time() - t0
                hh = hashlib.sha256()
                with open(out, "rb") as fi:
                    for chunk in iter(lambda: fi.read(1 << 24), b""):
                        hh.update(chunk)
                os.remove(out)
                digests.add(hh.hexdigest())
                rates.setdefault((t, setting), []).append(n / dt)
                print("round %d -t %2d %-6s: rc=%d wall %.2f s -> %.0f reads/s   tsv sha256 %s" % (rnd, t, setting, p.returncode, dt, n / dt, hh.hexdigest()[:16]), flush=True)
                if rnd == 0:
                    for line in p.stderr.decode().splitlines():
                        if "timing (reader" in line or ("inflate totals" in line and "fill 0.000" not in line):
                            print("   " + line.strip(), flush=True)
                    for line in [x for x in p.stderr.decode().splitlines() if "inflate round (device)" in x][1:5]:
                        print("   " + line.strip(), flush=True)
                if p.returncode:
                    sys.exit("charon dehost failed: " + p.stderr.decode()[-800:])
    for (t, setting), v in sorted(rates.items()):
        print("-t %2d %-6s: min %.0f  median %.0f  max %.0f reads/s over %d runs" % (t, setting, min(v), med(v), max(v), len(v)))
    print("TSV identical across runs: %s" % (len(digests) == 1))


if __name__ == "__main__":
    cmds = {"api": cmd_api, "cli": cmd_cli}
    if len(sys.argv) < 2 or sys.argv[1] not in cmds:
        sys.exit(__doc__)
    cmds[sys.argv[1]](sys.argv[2:])
