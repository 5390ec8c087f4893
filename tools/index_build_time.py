#!/usr/bin/env python3
"""How long does `charon index` take on references of some size?  Two synthetic genomes of N Mb each (one per category).
usage: python tools/index_build_time.py [Mb per genome] [workdir] [threads] [--legs NAME=EXE[@sets][@ef] ... [--rounds N]]

Without --legs: one run of this tree's binary, as ever.
With --legs: every leg is a binary (NAME=path of a `charon`), "@ef" behind the path runs it with CHARON_GPU_INDEX_EF=1 (the Elias-Fano arrays
encoded on the device), "@sets" with CHARON_GPU_INDEX_SETS=1 (the minimiser sets kept, sorted and made distinct in device memory); the two
combine ("@sets@ef"); without a suffix the variable is unset.  `threads` may be a comma list.  The legs run `--rounds` times (default 3) for every
thread count, the leg that goes first rotating from round to round; wall time and the last figure of the CHARON_TIMING line (the
"download + Elias-Fano" stage, whichever path ran), its "sort+unique" and its "minimisers" figures are reported as min - median - max, and
the sha256 of every file written."""
import hashlib, os, re, statistics, subprocess, sys, time
import numpy as np
argv = sys.argv[1:]
legs, rounds = [], 3
if "--legs" in argv:
    i = argv.index("--legs")
    rest, argv = argv[i + 1:], argv[:i]
    if "--rounds" in rest:
        j = rest.index("--rounds")
        rounds = int(rest[j + 1])
        rest = rest[:j] + rest[j + 2:]
    for spec in rest:
        name, exe = spec.split("=", 1)
        exe, *suffixes = exe.split("@")
        if set(suffixes) - {"ef", "sets"}:
            sys.exit("unknown suffix in " + spec)
        legs.append((name, exe, tuple(sorted(suffixes))))  # (what a leg switches on: "ef", "sets")
mb = int(argv[0]) if len(argv) > 0 else 200
work = argv[1] if len(argv) > 1 else "/tmp/charon_idx"
threads = argv[2] if len(argv) > 2 else "16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.makedirs(work, exist_ok=True)
r = np.random.default_rng(3)
acgt = np.frombuffer(b"ACGT", np.uint8)
with open(os.path.join(work, "refs.tsv"), "w") as tab:
    for name in ("microbial", "human"):
        fa = os.path.join(work, name + ".fa")
        with open(fa, "wb") as f:
            for c in range(mb // 50):  # chromosomes of 50 Mb, lines of 60 letters
                s = acgt[r.integers(0, 4, 50_000_000)]
                f.write(b">%s_chr%d\n" % (name.encode(), c))
                f.write(b"\n".join(s[i:i + 60].tobytes() for i in range(0, len(s), 60)) + b"\n")
        tab.write("%s\t%s\n" % (fa, name))


SWITCHES = {"ef": "CHARON_GPU_INDEX_EF", "sets": "CHARON_GPU_INDEX_SETS"}


def run(exe, nthreads, on=()):
    """one `charon index` run: (return code, wall seconds, stderr, log tail); the file is <work>/big.idx"""
    if os.path.exists(os.path.join(work, "big.idx")):
        os.remove(os.path.join(work, "big.idx"))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES.values()}
    env["CHARON_TIMING"] = "1"
    for sw in on:
        env[SWITCHES[sw]] = "1"
    t0 = time.time()
    p = subprocess.run([exe, "index", "-t", nthreads, "-p", os.path.join(work, "big"), "--log", os.path.join(work, "i.log"), os.path.join(work, "refs.tsv")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return p.returncode, time.time() - t0, p.stderr.decode(), open(os.path.join(work, "i.log")).read()[-600:]


if not legs:
    rc, dt, err, log = run(os.path.join(ROOT, "charon_amd", "bin", "charon"), threads)
    print("charon index -t %s: rc=%d, 2 x %d Mb in %.1f s (%.1f Mb/s), index file %.1f MB" % (threads, rc, mb, dt, 2 * mb / dt, os.path.getsize(os.path.join(work, "big.idx")) / 1e6 if rc == 0 else 0))
    print(err[-600:])
    print(log)
    sys.exit(0)

spread = lambda v: "%.3f - %.3f - %.3f" % (min(v), statistics.median(v), max(v))
hashes = set()
for nt in threads.split(","):
    wall = {name: [] for name, _, _ in legs}
    stage = {name: [] for name, _, _ in legs}
    sort_stage = {name: [] for name, _, _ in legs}
    min_stage = {name: [] for name, _, _ in legs}
    for rd in range(rounds):
        for name, exe, on in legs[rd % len(legs):] + legs[:rd % len(legs)]:
            rc, dt, err, _ = run(exe, nt, on)
            m = re.search(r"charon index: timing \(s\):.*minimisers \(device \+ download\) ([0-9.]+)  sort\+unique ([0-9.]+) .* ([0-9.]+)\s*$", err, re.M)
            if rc != 0 or not m:
                print("leg %s -t %s round %d: rc=%d\n%s" % (name, nt, rd, rc, err[-600:]))
                sys.exit(1)
            sha = hashlib.sha256(open(os.path.join(work, "big.idx"), "rb").read()).hexdigest()
            hashes.add(sha)
            wall[name].append(dt)
            stage[name].append(float(m.group(3)))
            sort_stage[name].append(float(m.group(2)))
            min_stage[name].append(float(m.group(1)))
            print("  -t %s round %d %-8s wall %.3f s  minimisers %.3f s  sort+unique %.3f s  Elias-Fano %.3f s  sha256 %s  %.1f MB" %
                  (nt, rd, name, dt, float(m.group(1)), float(m.group(2)), float(m.group(3)), sha[:16], os.path.getsize(os.path.join(work, "big.idx")) / 1e6), flush=True)
    for name, _, _ in legs:
        print("-t %-3s %-8s wall (s) %s   minimisers (s) %s   sort+unique (s) %s   download + Elias-Fano stage (s) %s   [min - median - max of %d]" %
              (nt, name, spread(wall[name]), spread(min_stage[name]), spread(sort_stage[name]), spread(stage[name]), rounds))
print("sha256 of the files: %s" % ("one value, " + next(iter(hashes)) if len(hashes) == 1 else "%d DIFFERENT values" % len(hashes)))
sys.exit(0 if len(hashes) == 1 else 1)
