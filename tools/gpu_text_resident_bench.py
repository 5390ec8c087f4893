#!/usr/bin/env python3
"""CLI comparison for CHARON_GPU_TEXT=1: `charon dehost` on two BGZF files -- the 7d file (synthetic reads of 5 kb, level 6)
and a nanopore-like set (500 b .. 50 kb, log-uniform) -- at every -t, in alternated rounds of four builds:
    parent                 PARENT_CHARON=<the parent commit's charon binary> (left out when unset)
    unset                  this build, no switch
    CHARON_GPU_INFLATE=1   this build, members inflated on the device, text downloaded
    CHARON_GPU_TEXT=1      this build, text stays in device memory
The sha256 of the TSV must be the same in every run of a file.  Prints, and writes to the output file, min-max reads/s per build and -t
and the CHARON_TIMING lines of the last round.  "unset" must lie inside the parent's range.
usage: python tools/gpu_text_resident_bench.py [reads=400000] [work dir] [rounds=3] [out=profiles/r09/gpu_text_resident.txt] [-t values...]

The paired leg (CHARON_GPU_TEXT_PAIRS=1): two BGZF files of 2 x 150 b pairs, in alternated rounds of parent, unset and
CHARON_GPU_TEXT=1 CHARON_GPU_TEXT_PAIRS=1; the same checks, pairs/s instead of reads/s.
usage: python tools/gpu_text_resident_bench.py pairs [pairs=4000000] [work dir] [rounds=3] [out=profiles/r10/gpu_text_pairs.txt] [-t values...]

The extract leg (CHARON_GPU_EXTRACT=1): `charon dehost --extract all` on the 7d file, in alternated rounds of the parent build
and this build with CHARON_GPU_TEXT=1 CHARON_GPU_DEFLATE=1, and this build with CHARON_GPU_EXTRACT=1 added.  The TSV and every extract
file must have one sha256 across the three.
usage: python tools/gpu_text_resident_bench.py extract [reads=400000] [work dir] [rounds=3] [out=profiles/r11/gpu_extract.txt] [-t values...]

--parent-switches (anywhere on the command line, with PARENT_CHARON set): every build with switches gets a twin "parent, <name>", the
parent binary under the same switches, and per -t a line saying whether this build's range overlaps its twin's -- or, where it lies
below, by how much of the twin's own min-max width.  For a change that claims only to be no slower than the parent in every mode."""
import hashlib
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCHES = ("CHARON_GPU_TEXT", "CHARON_GPU_TEXT_PAIRS", "CHARON_GPU_INFLATE", "CHARON_TEXT_BATCHES", "CHARON_GPU_DEFLATE", "CHARON_GPU_EXTRACT")


def sha256_of(path):
    hsh = hashlib.sha256()
    with open(path, "rb") as fi:
        for chunk in iter(lambda: fi.read(1 << 24), b""):
            hsh.update(chunk)
    return hsh.hexdigest()


def write_nanopore_like(path, letters, genomes, seed=2):
    """reads of 500 .. 50 000 letters, log-uniform, `letters` letters in all; returns the number of reads"""
    r = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    n = done = 0
    with open(path, "wb") as f:
        while done < letters:
            L = int(np.exp(r.uniform(np.log(500), np.log(50000))))
            g = genomes[n % len(genomes)]
            at = int(r.integers(0, len(g) - L))
            s = np.frombuffer(g, np.uint8)[at:at + L].copy()
            hit = r.random(L) < 0.05
            s[hit] = acgt[r.integers(0, 4, int(hit.sum()))]
            q = (r.integers(5, 41, L) + 33).astype(np.uint8)
            f.write(b"@n%09d\n" % n + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
            n += 1
            done += L
    return n


def write_pairs(paths, n, genomes, length=150, seed=3, chunk=20000):
    """n pairs of 2 x `length` letters: mate 1 and the reverse strand's start of a 400 b fragment, 3 % substitutions; ids p<i>/1, p<i>/2"""
    r = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    gsa = [np.frombuffer(g, np.uint8) for g in genomes]
    with open(paths[0], "wb") as f1, open(paths[1], "wb") as f2:
        for lo in range(0, n, chunk):
            m = min(chunk, n - lo)
            out = ([], [])
            for i in range(m):
                g = gsa[(lo + i) % len(gsa)]
                at = int(r.integers(0, len(g) - 400))
                frag = g[at:at + 400]
                for k, s in ((0, frag[:length].copy()), (1, comp[frag[::-1][:length]])):
                    hit = r.random(length) < 0.03
                    s[hit] = acgt[r.integers(0, 4, int(hit.sum()))]
                    q = (r.integers(5, 41, length) + 33).astype(np.uint8)
                    out[k].append(b"@p%09d/%d\n" % (lo + i, k + 1) + s.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
            f1.write(b"".join(out[0]))
            f2.write(b"".join(out[1]))


def main():
    twins = "--parent-switches" in sys.argv
    if twins:
        sys.argv.remove("--parent-switches")
    paired = len(sys.argv) > 1 and sys.argv[1] == "pairs"
    extract = len(sys.argv) > 1 and sys.argv[1] == "extract"
    if paired or extract:
        del sys.argv[1]
    n = int(sys.argv[1]) if len(sys.argv) > 1 else (4000000 if paired else 400000)
    work = sys.argv[2] if len(sys.argv) > 2 else "/tmp/charon_gpu_text_resident"
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    report = sys.argv[4] if len(sys.argv) > 4 else (os.path.join(ROOT, "profiles", "r10", "gpu_text_pairs.txt") if paired else
                                                     os.path.join(ROOT, "profiles", "r11", "gpu_extract.txt") if extract else
                                                     os.path.join(ROOT, "profiles", "r09", "gpu_text_resident.txt"))
    threads = [int(x) for x in sys.argv[5:]] or [1, 16]
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
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    files = []
    unit = "pairs/s" if paired else "reads/s"
    if paired:
        fqs = [os.path.join(work, "pairs_%d.fastq" % k) for k in (1, 2)]
        write_pairs(fqs, n, gs)
        for fq in fqs:
            subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_bgzf.py"), fq, fq + ".gz", "6", "16"], check=True)
        say("2 x 150 b pairs: %d pairs, %.2f GB of text, %.2f GB as BGZF" % (n, sum(os.path.getsize(fq) for fq in fqs) / 1e9,
                                                                            sum(os.path.getsize(fq + ".gz") for fq in fqs) / 1e9))
        for fq in fqs:
            os.remove(fq)
        files.append(("2 x 150 b pairs", [fq + ".gz" for fq in fqs], n))
    for label in (() if paired else ("5 kb reads", ) if extract else ("5 kb reads", "nanopore-like reads")):
        fq = os.path.join(work, "reads%d.fastq" % len(files))
        if not files:
            css.write_fastq(fq, n, gs)
            count = n
        else:
            count = write_nanopore_like(fq, n * css.L, gs)
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_bgzf.py"), fq, fq + ".gz", "6", "16"], check=True)
        say("%s: %d reads, %.2f GB of text, %.2f GB as BGZF" % (label, count, os.path.getsize(fq) / 1e9, os.path.getsize(fq + ".gz") / 1e9))
        os.remove(fq)
        files.append((label, [fq + ".gz"], count))

    parent = os.environ.get("PARENT_CHARON")
    base = {"CHARON_GPU_TEXT": "1", "CHARON_GPU_DEFLATE": "1"}
    configs = ([("parent, TEXT + DEFLATE", parent, base)] if parent else []) + [("TEXT + DEFLATE", exe, base), ("CHARON_GPU_EXTRACT=1", exe, dict(base, CHARON_GPU_EXTRACT="1"))]
    more = ["--extract", "all", "-p", os.path.join(work, "ex")] if extract else []
    configs = configs if extract else (([("parent", parent, {})] if parent else []) +
               [("unset", exe, {})] +
               ([("CHARON_GPU_TEXT_PAIRS=1", exe, {"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_PAIRS": "1"})] if paired else
                [("CHARON_GPU_INFLATE=1", exe, {"CHARON_GPU_INFLATE": "1"}), ("CHARON_GPU_TEXT=1", exe, {"CHARON_GPU_TEXT": "1"})]))
    if twins and parent:
        configs = [c for name, binary, extra in configs
                   for c in ([("parent, " + name, parent, extra)] if extra and binary == exe and ("parent, " + name, parent, extra) not in configs else []) + [(name, binary, extra)]]
    ok = True
    for label, bgzf, count in files:
        digests, rates, timing = set(), {}, {}
        for rnd in range(rounds):
            for t in threads:
                for name, binary, extra in configs:
                    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
                    env["CHARON_TIMING"] = "1"
                    env.update(extra)
                    out = os.path.join(work, "out.tsv")
                    t0 = time.time()
                    with open(out, "wb") as fo:
                        p = subprocess.run([binary, "dehost", "--db", os.path.join(work, "bench.idx"), "-t", str(t), "--log", os.path.join(work, "c.log")] + more + bgzf,
                                           stdout=fo, stderr=subprocess.PIPE, env=env, timeout=900)
                    dt = time.time() - t0
                    if p.returncode:
                        sys.exit("charon dehost failed (%s): %s" % (name, p.stderr.decode()[-800:]))
                    digest = sha256_of(out)
                    os.remove(out)
                    for x in sorted(os.listdir(work)) if extract else ():  # the extract files: <prefix>_<category>.fastq.gz
                        if x.startswith("ex_") and x.endswith(".gz"):
                            digest += " " + x + ":" + sha256_of(os.path.join(work, x))
                            os.remove(os.path.join(work, x))
                    digests.add(digest)
                    rates.setdefault((name, t), []).append(count / dt)
                    timing[(name, t)] = [ln.strip() for ln in p.stderr.decode().splitlines() if "timing (reader" in ln or "timing (main" in ln or "timing (CHARON_GPU_" in ln]
                    print("%s round %d %-24s -t %2d: %.2f s -> %.0f %s  sha256 %s" % (label, rnd, name, t, dt, count / dt, unit, digest[:16]), flush=True)
        say("")
        say("%s: TSV%s identical across runs: %s" % (label, " and extract files" if extract else "", len(digests) == 1))
        ok = ok and len(digests) == 1
        for (name, t), v in sorted(rates.items(), key=lambda kv: (kv[0][1], kv[0][0])):
            say("%-24s -t %2d: %.0f - %.0f %s over %d runs" % (name, t, min(v), max(v), unit, len(v)))
        for t in threads:
            if parent and not extract:
                u, pr = rates[("unset", t)], rates[("parent", t)]
                say("-t %d: unset inside the parent's range: %s" % (t, min(pr) <= max(u) and min(u) <= max(pr)))
            for name, _, _ in configs if twins and parent else ():
                if ("parent, " + name, t) in rates:
                    v, pv = rates[(name, t)], rates[("parent, " + name, t)]
                    width = max(pv) - min(pv)
                    if min(pv) <= max(v) and min(v) <= max(pv):
                        say("-t %d: %s overlaps its parent twin's range: True" % (t, name))
                    elif min(v) > max(pv):
                        say("-t %d: %s overlaps its parent twin's range: False (faster throughout: its minimum lies %.0f %s above the twin's maximum)"
                            % (t, name, min(v) - max(pv), unit))
                    else:
                        gap = min(pv) - max(v)
                        say("-t %d: %s overlaps its parent twin's range: False (its maximum lies %.0f %s below the twin's minimum; the twin's width is %.0f: %s)"
                            % (t, name, gap, unit, width, "within" if gap <= width else "NOT within"))
            for name, _, _ in configs:
                for ln in timing[(name, t)]:
                    say("   %-24s -t %2d %s" % (name, t, ln))
    os.makedirs(os.path.dirname(report), exist_ok=True)
    with open(report, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
