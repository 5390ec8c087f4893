#!/usr/bin/env python3
"""Steady-state throughput of `charon dehost` with and without CHARON_DEVICES, runs alternated in one session.

The workload of tools/cli_steady_state.py (5 kb reads from two 2 Mb genomes, index by this build's `charon index`); for every round, every
-t and every setting in turn: unset, CHARON_DEVICES=0, CHARON_DEVICES=0,0 (two replicas on one GPU).
usage: python tools/cli_devices_steady.py [n_reads] [workdir] [rounds] [threads ...]
With PARENT_CHARON=<path of another build's charon> that binary runs too (setting "parent", CHARON_DEVICES unset): the A/B of a change.
Prints wall time and reads/s of each run, the per-replica timers (CHARON_TIMING), the spread per (setting, -t) and whether every run wrote
the same TSV (sha256)."""
import hashlib
import importlib.util
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = (None, "0", "0,0")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4000000
    work = sys.argv[2] if len(sys.argv) > 2 else "/tmp/charon_cli_devices"
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    threads = [int(x) for x in sys.argv[4:]] or [1, 16]
    spec = importlib.util.spec_from_file_location("cli_steady_state", os.path.join(ROOT, "tools", "cli_steady_state.py"))
    css = importlib.util.module_from_spec(spec)
    sys.modules["cli_steady_state"] = css  # (its pool of writers pickles the module's block function by name)
    spec.loader.exec_module(css)
    os.makedirs(work, exist_ok=True)
    st = os.statvfs(work)
    free = st.f_bavail * st.f_frsize
    if n * css.REC * 1.3 > free:
        n2 = int(free / 1.3 / css.REC)
        print("only %.0f GB free under %s: %d reads instead of %d" % (free / 1e9, work, n2, n), flush=True)
        n = n2
    sys.path.insert(0, ROOT)
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
    print("fastq: %d reads of %d bases, %.1f GB, written in %.0f s" % (n, css.L, os.path.getsize(fq) / 1e9, time.time() - t0), flush=True)
    digests, rates = set(), {}
    parent = os.environ.get("PARENT_CHARON")
    for rnd in range(rounds):
        for t in threads:
            for dv in ((["parent"] if parent else []) + list(SETTINGS)):
                env = {k: v for k, v in os.environ.items() if k != "CHARON_DEVICES"}
                env["CHARON_TIMING"] = "1"
                if dv is not None and dv != "parent":
                    env["CHARON_DEVICES"] = dv
                out = os.path.join(work, "out.tsv")
                t0 = time.time()
                with open(out, "wb") as fo:
                    p = subprocess.run([parent if dv == "parent" else exe, "dehost", "--db", os.path.join(work, "bench.idx"), "-t", str(t), "--log", os.path.join(work, "c.log"), fq],
                                       stdout=fo, stderr=subprocess.PIPE, env=env, timeout=600)
                dt = time.time() - t0
                h = hashlib.sha256()
                with open(out, "rb") as fi:
                    for chunk in iter(lambda: fi.read(1 << 24), b""):
                        h.update(chunk)
                os.remove(out)
                digests.add(h.hexdigest())
                name = "unset" if dv is None else dv
                rates.setdefault((name, t), []).append(n / dt)
                print("round %d CHARON_DEVICES=%-5s -t %2d: rc=%d wall %.2f s -> %.0f reads/s   tsv sha256 %s" % (rnd, name, t, p.returncode, dt, n / dt, h.hexdigest()[:16]),
                      flush=True)
                for line in p.stderr.decode().splitlines():
                    if "timing (main" in line or "timing (replica" in line:
                        print("   " + line.strip(), flush=True)
                if p.returncode:
                    sys.exit("charon dehost failed: " + p.stderr.decode()[-800:])
    for (name, t), v in sorted(rates.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print("CHARON_DEVICES=%-5s -t %2d: min %.0f  median %.0f  max %.0f reads/s over %d runs" % (name, t, min(v), sorted(v)[len(v) // 2], max(v), len(v)))
    print("TSV identical across runs: %s" % (len(digests) == 1))


if __name__ == "__main__":
    main()
