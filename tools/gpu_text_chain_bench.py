#!/usr/bin/env python3
"""Two ways from BGZF members to waited per-read results, on the synthetic set of tools/gpu_inflate_bench.py (5 kb reads from two
2 Mb genomes, BGZF level 6).  Needs an MI355X.

usage: python tools/gpu_text_chain_bench.py [n_reads] [workdir] [reps]
  (a) today's composition: chn_inflate_run_crc into page-locked host memory, then chn_text_submit from that memory, then the wait;
      the records are found on the host in between (chn_text_split_host, one thread) -- timed, and listed on a line of its own;
  (b) the device chain: chn_inflate_run_crc with CHN_INFLATE_OUT_DEVICE, chn_text_split, chn_text_submit with CHN_TEXT_ON_DEVICE, the
      wait.  Both submit the same descriptors (those of (b)'s split; the host split's are checked to be the same).
Per stage: wall time of the call (min / median / max over the repetitions, the first one not counted: it allocates) and the device
time of its kernels from events (chn_inflate_kernel_ms; chn_stream_profile 6, 7, 8); bytes moved each way per read; whether both
ways gave the same results.  Everything is printed; nothing is asserted."""
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


def line(name, wall, kern=None):
    k = "" if kern is None else "   kernels median %8.3f ms" % med(kern)
    print("   %-46s wall min %8.3f median %8.3f max %8.3f ms%s" % (name, min(wall), med(wall), max(wall), k), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    work = sys.argv[2] if len(sys.argv) > 2 else "/tmp/charon_gpu_text_chain"
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    import charon_amd.api as api
    from tests import util
    spec = importlib.util.spec_from_file_location("cli_steady_state", os.path.join(ROOT, "tools", "cli_steady_state.py"))
    css = importlib.util.module_from_spec(spec)
    sys.modules["cli_steady_state"] = css  # (its pool of writers pickles the module's block function by name)
    spec.loader.exec_module(css)
    spec = importlib.util.spec_from_file_location("gpu_inflate_bench", os.path.join(ROOT, "tools", "gpu_inflate_bench.py"))
    gib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gib)
    os.makedirs(work, exist_ok=True)
    r = util.rng(1)
    gs = [util.random_seq(r, 2_000_000), util.random_seq(r, 2_000_000)]
    fq, bgzf = os.path.join(work, "reads.fastq"), os.path.join(work, "reads.fastq.gz")
    css.write_fastq(fq, n, gs)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_bgzf.py"), fq, bgzf, "6", "16"], check=True)
    text_bytes, comp_bytes = os.path.getsize(fq), os.path.getsize(bgzf)
    os.remove(fq)
    every = gib.bgzf_members(bgzf, 1 << 30)
    members, sizes, crcs = [m for m, _, _ in every], [s for _, s, _ in every], [c for _, _, c in every]
    assert sum(sizes) == text_bytes
    print("%d reads of %d bases: %.1f MB of text, %.1f MB as BGZF in %d members" % (n, css.L, text_bytes / 1e6, comp_bytes / 1e6, len(members)), flush=True)

    # an index of the bench's shape (what is in it does not matter here: both ways run the same chain on the same reads)
    index = api.Index(api.make_desc(2, 1 << 24, [0, 1], 2, 0))
    index.synth_fill(43, 0.215)
    st = api.Stream(index, n, n * ((css.L + 63) // 64 * 64), profile=True)
    st.set_model(api.default_model(2, 0))
    inf = api.Inflater(0)
    comp = np.zeros(n, np.float32)

    # (a): page-locked input and output
    ja, aa = api.inflate_job(members, sizes)
    pin_in, pin_out = api.pinned_array(aa["data"].size, np.uint8), api.pinned_array(text_bytes + 16, np.uint8)
    pin_in[:] = aa["data"]
    ja.in_, ja.out = pin_in.ctypes.data, pin_out.ctypes.data
    ca, caa = api.inflate_crc(len(members), crcs)
    # (b): page-locked input, device output
    dev_bytes = (text_bytes + 15) & ~15
    dev = api.device_malloc(0, dev_bytes)
    jb, ab = api.inflate_job(members, sizes, out_device=(dev, dev_bytes))
    jb.in_ = pin_in.ctypes.data
    cb, cab = api.inflate_crc(len(members), crcs)

    t = {k: [] for k in ("a_inflate", "a_split_host", "a_submit", "a_wait", "b_inflate", "b_split", "b_submit", "b_wait")}
    k = {key: [] for key in ("a_inflate", "a_upload", "a_pack", "b_inflate", "b_split", "b_pack")}
    res = {}
    for i in range(reps + 1):
        keep = i > 0
        now = time.perf_counter
        # ---- (b) ----
        t0 = now(); inf.run_job(jb, cb); t1 = now()
        kb_inf = inf.kernel_ms()
        sp = st.text_split(dev, text_bytes, max_records=n, ids_capacity=64 * n); t2 = now()
        tb = dict(seq1_offset=sp["seq_offset"], seq1_length=sp["seq_length"], qual1_offset=sp["qual_offset"], qual1_length=sp["seq_length"])
        t3 = now(); st.submit_text(tb, comp, text_device=(dev, text_bytes)); t4 = now()
        res["b"] = st.wait_text(); t5 = now()
        assert not ab["status"][:len(members)].any() and sp["n_records"] == n and sp["consumed"] == text_bytes
        prof_b = (st.profile(8, reset=True)[0], st.profile(6, reset=True)[0], st.profile(7, reset=True)[0])
        if keep:
            for key, v in (("b_inflate", t1 - t0), ("b_split", t2 - t1), ("b_submit", t4 - t3), ("b_wait", t5 - t4)):
                t[key].append(v * 1e3)
            k["b_inflate"].append(kb_inf); k["b_split"].append(prof_b[0]); k["b_pack"].append(prof_b[2])
        # ---- (a) ----
        t0 = now(); inf.run_job(ja, ca); t1 = now()
        ka_inf = inf.kernel_ms()
        hs = api.text_split_host(pin_out, max_records=n, ids_capacity=64 * n, nbytes=text_bytes); t2 = now()
        ta = dict(tb, text=pin_out, text_bytes=text_bytes)
        t3 = now(); st.submit_text(ta, comp); t4 = now()
        res["a"] = st.wait_text(); t5 = now()
        assert not aa["status"][:len(members)].any()
        prof_a = (st.profile(6, reset=True)[0], st.profile(7, reset=True)[0])
        if keep:
            for key, v in (("a_inflate", t1 - t0), ("a_split_host", t2 - t1), ("a_submit", t4 - t3), ("a_wait", t5 - t4)):
                t[key].append(v * 1e3)
            k["a_inflate"].append(ka_inf); k["a_upload"].append(prof_a[0]); k["a_pack"].append(prof_a[1])
        if i == 0:
            same_split = all(np.array_equal(hs[key], sp[key]) for key in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset")) and hs["ids"] == sp["ids"]
            same = all(np.array_equal(res["a"][key], res["b"][key], equal_nan=True) for key in ("num_hashes", "counts", "unique", "call", "conf", "probs", "mean_quality"))
            print("host split == device split: %s; results of (a) == results of (b): %s" % (same_split, same), flush=True)

    print("(a) inflate to page-locked host memory, submit from it")
    line("chn_inflate_run_crc (upload, decode, download)", t["a_inflate"], k["a_inflate"])
    line("chn_text_submit (text upload + pack, waited)", t["a_submit"], [x + y for x, y in zip(k["a_upload"], k["a_pack"])])
    print("      of those kernels' time: text upload median %.3f ms, k_text_pack + k_text_mq median %.3f ms" % (med(k["a_upload"]), med(k["a_pack"])))
    line("chn_text_wait", t["a_wait"])
    total_a = [a + b + c for a, b, c in zip(t["a_inflate"], t["a_submit"], t["a_wait"])]
    line("(a) members -> waited results, split not counted", total_a)
    line("records found on the host (chn_text_split_host)", t["a_split_host"])
    line("(a) with the host split", [a + b for a, b in zip(total_a, t["a_split_host"])])
    print("(b) inflate to device memory, split there, submit from there")
    line("chn_inflate_run_crc, CHN_INFLATE_OUT_DEVICE", t["b_inflate"], k["b_inflate"])
    line("chn_text_split (kernels, two waits, downloads)", t["b_split"], k["b_split"])
    line("chn_text_submit, CHN_TEXT_ON_DEVICE (pack, waited)", t["b_submit"], k["b_pack"])
    line("chn_text_wait", t["b_wait"])
    total_b = [a + b + c + d for a, b, c, d in zip(t["b_inflate"], t["b_split"], t["b_submit"], t["b_wait"])]
    line("(b) members -> waited results", total_b)
    print("medians: (a) %.1f ms = %.0f reads/s; (a) with the host split %.1f ms = %.0f reads/s; (b) %.1f ms = %.0f reads/s" %
          (med(total_a), n / med(total_a) * 1e3, med(total_a) + med(t["a_split_host"]), n / (med(total_a) + med(t["a_split_host"])) * 1e3,
           med(total_b), n / med(total_b) * 1e3))
    # bytes over PCIe per read (results: num_hashes 4, counts and unique 2 x 4 x 2 categories, probabilities 2 x 8, call, conf, flags, mean quality 4)
    result = 4 + 16 + 16 + 3 + 4
    padded = sum((len(m) + 15) & ~15 for m in members) + 128
    desc_up = len(members) * 28 + n * (8 + 4 + 8 + 4 + 8 + 4)  # member descriptors and expected CRCs; the text batch's offsets and lengths (+ segment offsets)
    up_a, down_a = padded + desc_up + text_bytes, text_bytes + len(members) * 8 + n * result
    up_b, down_b = padded + desc_up, len(members) * 8 + n * 32 + sp["ids_bytes"] + 32 + n * result
    print("bytes per read, host -> device: (a) %.0f (compressed %.0f, text %.0f, descriptors %.0f)   (b) %.0f (compressed %.0f, descriptors %.0f)" %
          (up_a / n, padded / n, text_bytes / n, desc_up / n, up_b / n, padded / n, desc_up / n))
    print("bytes per read, device -> host: (a) %.0f (text %.0f, statuses + CRCs %.1f, results %d)   (b) %.0f (record descriptors 32, ids %.1f, statuses + CRCs %.1f, results %d)" %
          (down_a / n, text_bytes / n, len(members) * 8 / n, result, down_b / n, sp["ids_bytes"] / n, len(members) * 8 / n, result))
    st.destroy()
    inf.destroy()
    index.destroy()
    api.device_free(0, dev)
    api.host_free(pin_in)
    api.host_free(pin_out)


if __name__ == "__main__":
    main()
