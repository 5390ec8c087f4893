#!/usr/bin/env python3
"""Measurements of text batches (chn_text_submit / k_text_pack, CHARON_TEXT_BATCHES=1).  Needs an MI355X.

  python tools/text_batch_bench.py pack   [reps]
      k_text_pack (+ the mean-quality division) against the host -> device copy of the same batch's text out of page-locked memory,
      both timed with HIP events on the copy stream in the same call (chn_stream_profile 6 / 7), for three shapes:
      65 536 x 5 kb reads, 1 M pairs of 2 x 150 b, 2 000 reads log-uniform in 500 b - 1 Mb.  Requirement: pack <= copy.
  python tools/text_batch_bench.py flight [n_reads] [steps] [blocks]
      three batches in flight of n_reads x 5 kb reads against the bench's cfg2-shaped index: text batches against host-packed batches
      (packing excluded for the latter), alternated block by block in one process; spread first.
  python tools/text_batch_bench.py cli    [n_reads] [workdir] [rounds] [threads ...]
      `charon dehost` on plain FASTQ, one-stream .gz and BGZF of n_reads x 5 kb reads: PARENT_CHARON=<another build's charon> (if
      set), this build with the switch unset, and with CHARON_TEXT_BATCHES=1, alternated; TSV sha256 of every run; per-phase times
      (CHARON_TIMING) of the .gz runs.  TEXT_BENCH_SETTINGS / TEXT_BENCH_INPUTS (comma lists of parent, unset, text / plain, gz, bgzf) narrow the runs.
Everything is printed; nothing is asserted."""
import ctypes as C
import hashlib
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return sorted(v)[len(v) // 2]


def pinned_copy(api, arr):
    p = api.pinned_array(arr.shape, arr.dtype)
    p[...] = arr
    return p


def fastq_like(r, len1, len2=None):
    """a text batch laid out like FASTQ records (a 7-byte id line, the letters, '\\n+\\n', the qualities, '\\n'); every byte of the
    buffer is a random letter of ACGT (the pack kernel does not look at quality values, nor at what lies between the stretches)"""
    n = len(len1)
    cols = [("seq1", len1), ("qual1", len1)] + ([("seq2", len2), ("qual2", len2)] if len2 is not None else [])
    gaps = [7, 3, 8, 3]
    rec = sum(int(g) for g in gaps[:len(cols)]) + 1
    per = sum(c[1].astype(np.int64) for c in cols) + rec
    start = np.concatenate([[0], np.cumsum(per)[:-1]]).astype(np.int64)
    tb, cur = dict(flags=0), start.copy()
    for (name, ln), g in zip(cols, gaps):
        cur = cur + g
        tb[name + "_offset"] = cur.astype(np.uint64)
        tb[name + "_length"] = ln.astype(np.uint32)
        cur = cur + ln.astype(np.int64)
    total = int(per.sum())
    tb["text"] = np.frombuffer(b"ACGT", np.uint8)[r.integers(0, 4, total, dtype=np.uint8)]
    return tb, total


def cmd_pack(argv):
    import charon_amd.api as api
    reps = int(argv[0]) if argv else 7
    r = np.random.default_rng(5)
    shapes = [("65 536 x 5 kb", np.full(65536, 5000, np.uint32), None),
              ("1 M pairs of 2 x 150 b", np.full(1 << 20, 150, np.uint32), np.full(1 << 20, 150, np.uint32)),
              ("2 000 reads log-uniform 500 b - 1 Mb", np.exp(r.uniform(np.log(500), np.log(1e6), 2000)).astype(np.uint32), None)]
    index = api.Index(api.make_desc(2, 1 << 16, [0, 1], 2, 0))
    L = api.lib()
    for name, l1, l2 in shapes:
        tb, total = fastq_like(r, l1, l2)
        tb["text"] = pinned_copy(api, tb["text"])
        pad = lambda x: (x.astype(np.int64) + 63) // 64 * 64
        n_bases = int(pad(l1).sum() + (pad(l2).sum() if l2 is not None else 0))
        st = api.Stream(index, len(l1), n_bases, profile=True)
        t, keep, n = st._text_batch(tb)
        nb, hn = C.c_uint64(), C.c_uint32()
        up, pk = [], []
        for i in range(reps + 1):
            api._chk(L.chn_text_pack(st.h, C.byref(t), None, None, None, None, None, C.byref(nb), C.byref(hn)))
            a, b = st.profile(6, reset=True)[0], st.profile(7, reset=True)[0]
            if i:  # the first call allocates
                up.append(a)
                pk.append(b)
        letters = int(l1.sum()) + (int(l2.sum()) if l2 is not None else 0)
        print("%-38s text %7.1f MB, %6.1f M letters: copy min %.3f median %.3f max %.3f ms (%.1f GB/s); pack min %.3f median %.3f max %.3f ms "
              "(%.0f G letters/s, %.2f of the copy) -> pack <= copy: %s" %
              (name, total / 1e6, letters / 1e6, min(up), med(up), max(up), total / med(up) / 1e6, min(pk), med(pk), max(pk), letters / med(pk) / 1e6,
               med(pk) / med(up), med(pk) <= med(up)), flush=True)
        st.destroy()
        api.host_free(tb["text"])
    index.destroy()


def cmd_flight(argv):
    import charon_amd.api as api
    n = int(argv[0]) if argv else 65536
    steps = int(argv[1]) if len(argv) > 1 else 12
    blocks = int(argv[2]) if len(argv) > 2 else 3
    Lr, B, S, glen = 5000, 2, 1 << 27, 1 << 24
    index = api.Index(api.make_desc(B, S, [0, 1], 2, 0))
    index.synth_fill(43, 0.215)
    genomes = api.synth_genomes(0, 43, B, glen)
    index.synth_plant(genomes, B, glen, list(range(B)))
    rd = api.synth_reads(0, 42, genomes, B, glen, n, Lr, Lr, 0.05, 0.10, 40.0)
    nb = int(rd.n_bases)
    bases2 = api.device_download(0, rd.bases2, nb // 4, np.uint32)
    off = api.device_download(0, rd.seg1_offset, n * 8, np.uint64)
    ln = api.device_download(0, rd.seg1_length, n * 4, np.uint32)
    # the same reads as text: unpack the codes, lay them out as FASTQ-like records with constant qualities
    stride = nb // n
    assert stride * n == nb and (ln == Lr).all()
    codes = np.empty(nb, np.uint8)
    for j in range(16):
        codes[j::16] = (bases2 >> np.uint32(2 * j)) & 3
    letters = np.frombuffer(b"ACGT", np.uint8)[codes].reshape(n, stride)[:, :Lr]
    rec = 12 + Lr + 3 + Lr + 1
    text = api.pinned_array((n, rec), np.uint8)
    text[:, :12] = np.frombuffer(b"@r000000000\n", np.uint8)
    text[:, 12:12 + Lr] = letters
    text[:, 12 + Lr:15 + Lr] = np.frombuffer(b"\n+\n", np.uint8)
    text[:, 15 + Lr:15 + 2 * Lr] = ord("I")
    text[:, rec - 1] = 10
    base = np.arange(n, dtype=np.uint64) * np.uint64(rec)
    tb = dict(flags=0, text=text.reshape(-1), seq1_offset=base + np.uint64(12), seq1_length=ln, qual1_offset=base + np.uint64(15 + Lr), qual1_length=ln)
    packed = dict(bases2=pinned_copy(api, bases2), nmask=None, seg1_offset=off, seg1_length=ln, seg2_offset=None, seg2_length=None, n_bases=nb)
    mq, comp = np.full(n, 40.0, np.float32), np.zeros(n, np.float32)
    st = api.Stream(index, n, nb)
    st.set_model(api.default_model(2, 0))
    print("flight: %d reads x %d b, text %.1f MB per batch, packed %.1f MB per batch, three in flight, %d timed batches per block" %
          (n, Lr, text.size / 1e6, bases2.nbytes / 1e6, steps), flush=True)

    def run(kind):
        sub = (lambda: st.submit_text(tb, comp)) if kind == "text" else (lambda: st.submit_host(packed, mq, comp))
        wait = st.wait_text if kind == "text" else st.wait_host
        for _ in range(3):
            sub()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = wait()
            sub()
        dt = time.perf_counter() - t0
        for _ in range(3):
            out = wait()
        return n * steps / dt, out

    run("text"), run("packed")  # warm-up: allocations
    rates, ref = {"text": [], "packed": []}, {}
    for b in range(blocks):
        for kind in ("packed", "text"):
            rate, out = run(kind)
            rates[kind].append(rate)
            ref[kind] = out
            print("block %d %-6s: %.3f M reads/s (%.2f ms per batch)" % (b, kind, rate / 1e6, n / rate * 1e3), flush=True)
    same = all(np.array_equal(ref["text"][k], ref["packed"][k], equal_nan=True) for k in ("num_hashes", "counts", "unique", "call", "conf", "probs"))
    for kind, v in rates.items():
        print("%-6s: min %.3f median %.3f max %.3f M reads/s over %d blocks" % (kind, min(v) / 1e6, med(v) / 1e6, max(v) / 1e6, len(v)))
    print("text / packed (medians): %.3f; results identical: %s" % (med(rates["text"]) / med(rates["packed"]), same))
    st.destroy()
    index.destroy()


def cmd_cli(argv):
    n = int(argv[0]) if argv else 400000
    work = argv[1] if len(argv) > 1 else "/tmp/charon_text_cli"
    rounds = int(argv[2]) if len(argv) > 2 else 2
    threads = [int(x) for x in argv[3:]] or [1, 8, 16]
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
    subprocess.run("gzip -1 -c %s > %s" % (fq, os.path.join(work, "one.fastq.gz")), shell=True, check=True)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_bgzf.py"), fq, os.path.join(work, "bgzf.fastq.gz"), "1", "16"], check=True)
    inputs = [("plain", fq), ("gz", os.path.join(work, "one.fastq.gz")), ("bgzf", os.path.join(work, "bgzf.fastq.gz"))]
    print("inputs: %d reads of %d bases; plain %.2f GB, .gz %.2f GB, BGZF %.2f GB; prepared in %.0f s" %
          (n, css.L, os.path.getsize(fq) / 1e9, os.path.getsize(inputs[1][1]) / 1e9, os.path.getsize(inputs[2][1]) / 1e9, time.time() - t0), flush=True)
    parent = os.environ.get("PARENT_CHARON")
    settings = (["parent"] if parent else []) + ["unset", "text"]
    if os.environ.get("TEXT_BENCH_SETTINGS"):  # e.g. "parent,unset": the A/B of the default path alone, more rounds in the same time
        settings = [x for x in settings if x in os.environ["TEXT_BENCH_SETTINGS"].split(",")]
    if os.environ.get("TEXT_BENCH_INPUTS"):
        inputs = [x for x in inputs if x[0] in os.environ["TEXT_BENCH_INPUTS"].split(",")]
    digests, rates = set(), {}
    for rnd in range(rounds):
        for kind, path in inputs:
            for t in threads:
                for setting in settings:
                    env = {k: v for k, v in os.environ.items() if k != "CHARON_TEXT_BATCHES"}
                    env["CHARON_TIMING"] = "1"
                    if setting == "text":
                        env["CHARON_TEXT_BATCHES"] = "1"
                    out = os.path.join(work, "out.tsv")
                    t0 = time.time()
                    with open(out, "wb") as fo:
                        p = subprocess.run([parent if setting == "parent" else exe, "dehost", "--db", os.path.join(work, "bench.idx"), "-t", str(t), "--log",
                                            os.path.join(work, "c.log"), path], stdout=fo, stderr=subprocess.PIPE, env=env, timeout=900)
                    dt = time.time() - t0
                    h = hashlib.sha256()
                    with open(out, "rb") as fi:
                        for chunk in iter(lambda: fi.read(1 << 24), b""):
                            h.update(chunk)
                    os.remove(out)
                    digests.add(h.hexdigest())
                    rates.setdefault((kind, t, setting), []).append(n / dt)
                    print("round %d %-5s -t %2d %-6s: rc=%d wall %.2f s -> %.0f reads/s   tsv sha256 %s" % (rnd, kind, t, setting, p.returncode, dt, n / dt, h.hexdigest()[:16]),
                          flush=True)
                    if kind == "gz" and rnd == 0:
                        for line in p.stderr.decode().splitlines():
                            if "timing (main" in line or "timing (reader" in line or "timing (replica" in line:
                                print("   " + line.strip(), flush=True)
                    if p.returncode:
                        sys.exit("charon dehost failed: " + p.stderr.decode()[-800:])
    for (kind, t, setting), v in sorted(rates.items()):
        print("%-5s -t %2d %-6s: min %.0f  median %.0f  max %.0f reads/s over %d runs" % (kind, t, setting, min(v), med(v), max(v), len(v)))
    print("TSV identical across runs: %s" % (len(digests) == 1))


if __name__ == "__main__":
    cmds = {"pack": cmd_pack, "flight": cmd_flight, "cli": cmd_cli}
    if len(sys.argv) < 2 or sys.argv[1] not in cmds:
        sys.exit(__doc__)
    cmds[sys.argv[1]](sys.argv[2:])
