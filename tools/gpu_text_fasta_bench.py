#!/usr/bin/env python3
"""CLI comparison for CHARON_GPU_TEXT_FASTA=1: `charon dehost --min_quality 0` on synthetic reads of 5 kb as BGZF FASTA
(70-letter lines, level 6) at every -t, in alternated rounds of three builds:
    parent                       PARENT_CHARON=<the parent commit's charon binary> (left out when unset)
    unset                        this build, no switch
    CHARON_GPU_TEXT_FASTA=1      this build with CHARON_GPU_TEXT=1 CHARON_GPU_TEXT_FASTA=1: the text stays in device memory
The sha256 of the TSV must be the same in every run.  Prints, and writes to the output file, min-max reads/s per build and -t, the
CHARON_TIMING lines of the last round, and the event time of chn_fasta_split's kernels (chn_stream_profile slot 14) on the first
64 MiB of the text beside chn_fasta_split_host on the same bytes.
usage: python tools/gpu_text_fasta_bench.py [reads=400000] [work dir] [rounds=3] [out=profiles/r13/gpu_text_fasta.txt] [-t values...]"""
import hashlib
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCHES = ("CHARON_GPU_TEXT", "CHARON_GPU_TEXT_FASTA", "CHARON_GPU_TEXT_PAIRS", "CHARON_GPU_INFLATE", "CHARON_TEXT_BATCHES", "CHARON_GPU_DEFLATE",
            "CHARON_GPU_EXTRACT")
WIDTH = 70


def sha256_of(path):
    hsh = hashlib.sha256()
    with open(path, "rb") as fi:
        for chunk in iter(lambda: fi.read(1 << 24), b""):
            hsh.update(chunk)
    return hsh.hexdigest()


def fastq_to_fasta(css, fq, fa, chunk=20000):
    """the fixed-size records of cli_steady_state.write_fastq as FASTA in lines of WIDTH letters"""
    L, head = css.L, 2 + css.IDW + 1
    full, rest = divmod(L, WIDTH)
    rows = full + (1 if rest else 0)
    with open(fq, "rb") as fi, open(fa, "wb") as fo:
        while True:
            a = np.frombuffer(fi.read(chunk * css.REC), np.uint8)
            if not a.size:
                break
            a = a.reshape(-1, css.REC)
            m = a.shape[0]
            seq = np.full((m, rows * WIDTH), ord("A"), np.uint8)
            seq[:, :L] = a[:, head:head + L]
            lines = np.concatenate([seq.reshape(m, rows, WIDTH), np.full((m, rows, 1), 10, np.uint8)], axis=2).reshape(m, rows * (WIDTH + 1))
            out = np.concatenate([a[:, :head], lines[:, :full * (WIDTH + 1) + rest] if rest else lines, np.full((m, 1 if rest else 0), 10, np.uint8)], axis=1)
            out[:, 0] = ord(">")
            fo.write(out.tobytes())


def kernel_times(fa, say, block=64 << 20, calls=5):
    """chn_fasta_split on the first `block` bytes of the text: event time of its kernels per call, and the host twin on the same bytes"""
    import charon_amd.api as api
    from tests import util
    from oracle import pyoracle as po
    with open(fa, "rb") as f:
        text = np.frombuffer(f.read(block), np.uint8)
    r = util.rng(3)
    oidx = util.build_oracle_index(po, [[util.random_seq(r, 5000)], [util.random_seq(r, 5000)]], [0, 1], ["microbial", "host"])
    g = util.gpu_index_from_oracle(api, oidx)
    st = api.Stream(g, 1024, 1 << 20, profile=True)
    cap = (text.size + 15) & ~15
    dtext, dseq = api.device_malloc(0, cap), api.device_malloc(0, cap)
    try:
        api.device_upload(0, dtext, np.concatenate([text, np.full(cap - text.size, 10, np.uint8)]))
        max_records = text.size // 4000
        st.fasta_split(dtext, text.size, dseq, cap, max_records=max_records)  # (allocates the scratch)
        st.profile(14, reset=True)
        t0 = time.time()
        for _ in range(calls):
            got = st.fasta_split(dtext, text.size, dseq, cap, max_records=max_records)
        wall = (time.time() - t0) / calls
        ms, n = st.profile(14)
        t0 = time.time()
        want = api.fasta_split_host(text, max_records=max_records)
        host = time.time() - t0
        same = all(got[k] == want[k] for k in ("n_records", "consumed", "ids_bytes", "seq_bytes", "ids")) and \
            api.device_download(0, dseq, (got["seq_bytes"] + 15) & ~15, np.uint8)[:got["seq_bytes"]].tobytes() == want["seq_text"]
        say("chn_fasta_split on %.1f MiB of the text (%d records, %d letters): kernels %.3f ms a call by events (%.1f GB/s of text), the call %.3f ms by the clock; "
            "chn_fasta_split_host on the same bytes %.1f ms; outputs equal: %s" % (text.size / 2 ** 20, got["n_records"], got["seq_bytes"], ms / n, text.size / (ms / n) / 1e6,
                                                                                wall * 1e3, host * 1e3, same))
        return same
    finally:
        api.device_free(0, dtext)
        api.device_free(0, dseq)
        st.destroy()
        g.destroy()
        oidx.free()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
    work = sys.argv[2] if len(sys.argv) > 2 else "/tmp/charon_gpu_text_fasta"
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    report = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r13", "gpu_text_fasta.txt")
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

    fq, fa = os.path.join(work, "reads.fastq"), os.path.join(work, "reads.fasta")
    css.write_fastq(fq, n, gs)
    fastq_to_fasta(css, fq, fa)
    os.remove(fq)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_bgzf.py"), fa, fa + ".gz", "6", "16"], check=True)
    say("5 kb reads as FASTA in %d-letter lines: %d reads, %.2f GB of text, %.2f GB as BGZF" % (WIDTH, n, os.path.getsize(fa) / 1e9, os.path.getsize(fa + ".gz") / 1e9))
    ok = kernel_times(fa, say)
    os.remove(fa)

    parent = os.environ.get("PARENT_CHARON")
    configs = ([("parent", parent, {})] if parent else []) + [("unset", exe, {}), ("CHARON_GPU_TEXT_FASTA=1", exe, {"CHARON_GPU_TEXT": "1", "CHARON_GPU_TEXT_FASTA": "1"})]
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
                    p = subprocess.run([binary, "dehost", "--db", os.path.join(work, "bench.idx"), "--min_quality", "0", "-t", str(t), "--log", os.path.join(work, "c.log"),
                                        fa + ".gz"], stdout=fo, stderr=subprocess.PIPE, env=env, timeout=900)
                dt = time.time() - t0
                if p.returncode:
                    sys.exit("charon dehost failed (%s): %s" % (name, p.stderr.decode()[-800:]))
                if extra and "FASTA records are found and unwrapped on the device" not in open(os.path.join(work, "c.log")).read():
                    sys.exit("the switch did not apply (%s)" % name)
                digest = sha256_of(out)
                os.remove(out)
                digests.add(digest)
                rates.setdefault((name, t), []).append(n / dt)
                timing[(name, t)] = [ln.strip() for ln in p.stderr.decode().splitlines() if "timing (reader" in ln or "timing (main" in ln or "timing (CHARON_GPU_" in ln]
                print("round %d %-24s -t %2d: %.2f s -> %.0f reads/s  sha256 %s" % (rnd, name, t, dt, n / dt, digest[:16]), flush=True)
    say("")
    say("TSV identical across runs: %s" % (len(digests) == 1))
    ok = ok and len(digests) == 1
    for (name, t), v in sorted(rates.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        say("%-24s -t %2d: %.0f - %.0f reads/s over %d runs" % (name, t, min(v), max(v), len(v)))
    for t in threads:
        if parent:
            u, pr = rates[("unset", t)], rates[("parent", t)]
            say("-t %d: unset inside the parent's range: %s" % (t, min(pr) <= max(u) and min(u) <= max(pr)))
        for name, _, _ in configs:
            for ln in timing[(name, t)]:
                say("   %-24s -t %2d %s" % (name, t, ln))
    os.makedirs(os.path.dirname(report), exist_ok=True)
    with open(report, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
