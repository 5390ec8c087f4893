#!/usr/bin/env python3
"""`charon dehost` end to end with the default gzip routing (reads beyond 61 440 letters to the device's long-read deflate pass where
gzip_long_device_limit says it pays) against CHARON_GZIP_GPU_MAX=61440 (every such read on the host), alternating in one process, at
-t 1 and -t 16, on three inputs: nanopore-like reads (1 - 60 kb) with 200 ultra-long ones (100 kb - 2 Mb), the same with none, and
65 536 x 5 kb reads plus two 2 Mb reads.   usage: python tools/cli_gzip_long_routing.py [workdir] [repeats]"""
import os, re, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import util

work = sys.argv[1] if len(sys.argv) > 1 else "/tmp/charon_gzlong"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
os.makedirs(work, exist_ok=True)
r = util.rng(7)
gs = [util.random_seq(r, 4_000_000), util.random_seq(r, 4_000_000)]
exe = os.path.join(ROOT, "charon_amd", "bin", "charon")
with open(os.path.join(work, "refs.tsv"), "w") as tab:
    for name, g in (("microbial", gs[0]), ("human", gs[1])):
        fa = os.path.join(work, name + ".fa")
        open(fa, "wb").write(b">" + name.encode() + b"\n" + g + b"\n")
        tab.write("%s\t%s\n" % (fa, name))
if os.path.exists(os.path.join(work, "long.idx")):
    os.remove(os.path.join(work, "long.idx"))
subprocess.run([exe, "index", "-p", os.path.join(work, "long"), "--log", os.path.join(work, "i.log"), os.path.join(work, "refs.tsv")], check=True,
               stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def write(name, lens):
    fq = os.path.join(work, name)
    with open(fq, "wb") as f:
        for i, L in enumerate(lens):
            g = gs[i & 1]
            s = int(r.integers(0, len(g) - L))
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, util.mutate(r, g[s:s + L], 0.05), b"I" * int(L)))
    return fq


n = 60000
base = np.exp(r.uniform(np.log(1000), np.log(60000), n)).astype(int)
ultra = base.copy()
ultra[r.choice(n, 200, replace=False)] = np.exp(r.uniform(np.log(100000), np.log(2000000), 200)).astype(int)
lone = np.full(65536, 5000)
lone[[1000, 40000]] = 2000000
cases = [("60000 reads, 200 ultra-long", write("ultra.fq", ultra)), ("60000 reads, no ultra-long", write("plain.fq", base)),
         ("65536 x 5 kb + two 2 Mb", write("lone.fq", lone))]
for label, fq in cases:
    for t in (1, 16):
        times = {"default": [], "61440": []}
        ref = None
        for rep in range(reps):
            for setting in ("default", "61440"):
                env = dict(os.environ)
                if setting == "61440":
                    env["CHARON_GZIP_GPU_MAX"] = "61440"
                log = os.path.join(work, "c.log")
                t0 = time.time()
                p = subprocess.run([exe, "dehost", "--db", os.path.join(work, "long.idx"), "-t", str(t), "--log", log, fq], stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE, env=env)
                dt = time.time() - t0
                if p.returncode != 0:
                    sys.exit("charon failed: " + p.stderr.decode()[-2000:])
                ref = ref or p.stdout
                assert p.stdout == ref, (label, t, setting)
                m = re.findall(r"gzip column: (\d+) reads beyond", open(log).read())
                times[setting].append(dt)
                print("%-28s -t %2d %-8s %.3f s  long reads on the device: %s" % (label, t, setting, dt, m[-1] if m else "?"), flush=True)
        d, b = np.median(times["default"]), np.median(times["61440"])
        print("%-28s -t %2d median default %.3f s, median CHARON_GZIP_GPU_MAX=61440 %.3f s: ratio %.3f (identical TSV)" % (label, t, d, b, d / b), flush=True)
