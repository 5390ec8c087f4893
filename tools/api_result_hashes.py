#!/usr/bin/env python3
"""A fixed set of runs through the C ABI, one line per run: sha256 over every result column.  Two builds of libcharon_hip.so compute the
same if and only if their lines are equal: run it once per library (CHARON_HIP_LIB=/path/to/the/other/libcharon_hip.so) and diff.

The set: host and device batches, single and paired, on the fused and the row-log layouts (indices and read sets of
tests/test_gpu_device_batches.py); W = 1 .. 4 words per row with device-made reads; each gzip output mode; a CHN_STREAM_TINY_LOG
re-run; a SPLIT batch; the dense and the sparse row-sharded chains on one rank; a text batch; three batches in flight.
usage: python tools/api_result_hashes.py > hashes.txt"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import charon_amd.api as api  # noqa: E402
from charon_amd import pack  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import util  # noqa: E402
from tests import test_gpu_device_batches as dbt  # noqa: E402

KEYS = ("num_hashes", "counts", "unique", "probs", "call", "conf", "flags", "gzip_sizes", "gzip_tallies", "mean_quality")


def line(name, out):
    h = hashlib.sha256()
    cols = []
    for key in KEYS:
        if key in out:
            a = np.ascontiguousarray(out[key])
            if key == "gzip_tallies":
                a = np.ascontiguousarray(a[:, :317])  # (the pad behind the status word is not part of the result)
            h.update(key.encode() + a.tobytes())
            cols.append(key)
    print("%-44s %s  rows %6d  %s" % (name, h.hexdigest()[:32], len(out["num_hashes"]), ",".join(cols)), flush=True)


def stream(g, n, n_bases, paired, **kw):
    st = api.Stream(g, n, n_bases, **kw)
    st.set_model(dbt.model_for(api, g, paired))
    return st


def host_and_device(tag, g, reads, mates, **kw):
    n, paired = len(reads), mates is not None
    p, db = dbt.packed_and_device(api, reads, mates)
    st = stream(g, n, p["n_bases"], paired, **kw)
    st.submit_host(p, *dbt.host_columns(n))
    line(tag + " host", st.wait_host())
    db.submit(st)
    line(tag + " device", dbt.wait_downloaded(api, st, n))
    # three in flight, both forms
    st.submit_host(p, *dbt.host_columns(n)); db.submit(st); st.submit_host(p, *dbt.host_columns(n))
    line(tag + " in flight 1 (host)", st.wait_host())
    line(tag + " in flight 2 (device)", dbt.wait_downloaded(api, st, n))
    line(tag + " in flight 3 (host)", st.wait_host())
    reruns = st.profile(4)[1]
    st.destroy()
    db.free()
    return reruns


def main():
    po.build()
    gs = dbt.make_genomes()
    fused, rows = dbt.build_indices(po, gs)
    fused_se = util.build_oracle_index(po, [[g] for g in gs], list(range(8)), ["host"] + ["c%d" % i for i in range(7)])
    gf, gr, gse = (util.gpu_index_from_oracle(api, x) for x in (fused, rows, fused_se))
    sets = dbt.make_sets(gs)
    se, pairs, se_n = sets["se"], sets["pairs"], sets["se_n"]

    host_and_device("fused pairs", gf, *pairs)
    host_and_device("fused single", gse, *se)
    host_and_device("rows single", gr, *se)
    host_and_device("rows single with N", gr, *se_n)
    host_and_device("rows pairs", gr, *pairs)
    print("# re-runs: %d" % host_and_device("rows single, TINY_LOG", gr, *se, tiny_log=True))
    host_and_device("rows single, SPLIT from 1 024 bases", gr, *se, split_bucket=64)
    host_and_device("fused single, SPLIT from 1 024 bases", gse, *se, split_bucket=64)

    # every gzip output mode, host and device batches, a text batch
    gz = dbt.make_gzip_sets(gs)
    for name in ("se", "pairs", "bound_se", "bound_pairs"):
        reads, mates = gz[name]
        n = len(reads)
        p, db = dbt.packed_and_device(api, reads, mates)
        st = stream(gr, n, p["n_bases"], mates is not None)
        for mode, bound in ((api.GZIP_TALLIES, 16384), (api.GZIP_SIZES, 16384), (api.GZIP_BOTH, 2000), (api.GZIP_SIZES_ALL, api.GZIP_ANY_LEN), (api.GZIP_SIZES_ALL, 2000)):
            st.submit_host(p, np.full(n, 40.0, np.float32), None, gzip_tallies=bound, gzip_output=mode)
            line("gzip %s host mode %d bound %d" % (name, mode, bound), st.wait_host())
            if mode != api.GZIP_SIZES_ALL:
                db.submit(st, gzip_tallies=bound, gzip_output=mode)
                line("gzip %s device mode %d bound %d" % (name, mode, bound), dbt.wait_downloaded(api, st, n, gzip_output=mode))
        st.destroy()
        db.free()
    r = util.rng(7)
    long_reads = [util.random_seq(r, L) for L in (70000, 61440, 61441, 16383, 16384, 150, 90000, 70000)] + [gs[0][:1500] * 30]
    p = pack.pack_reads(long_reads)
    st = stream(gr, len(long_reads), p["n_bases"], False)
    st.submit_host(p, np.full(len(long_reads), 40.0, np.float32), None, gzip_tallies=api.GZIP_ANY_LEN, gzip_output=api.GZIP_SIZES_ALL)
    line("gzip long reads host mode 3", st.wait_host())
    st.destroy()

    reads = se[0]
    quals = [bytes(33 + (7 * i + j) % 40 for j in range(len(s))) for i, s in enumerate(reads)]
    st = stream(gr, len(reads), pack.pack_reads(reads)["n_bases"] + 64 * len(reads), False)
    st.submit_text(pack.text_batch(reads, quals, gap=b"\n+\n"), np.zeros(len(reads), np.float32))
    line("text batch", st.wait_text())
    st.submit_text(pack.text_batch(reads, quals, gap=b"\n+\n"), None, gzip_tallies=16384, gzip_output=api.GZIP_SIZES)
    line("text batch, gzip sizes", st.wait_text())
    st.destroy()

    # the dense row-sharded chain on one rank, and chn_minimisers
    n = len(reads)
    p, db = dbt.packed_and_device(api, reads)
    st = stream(gr, n, p["n_bases"], False)
    mins = st.minimisers_host(p)
    print("%-44s %s  values %d" % ("chn_minimisers", hashlib.sha256(np.sort(mins).tobytes()).hexdigest()[:32], mins.size), flush=True)
    e = st.shard_minimise_device(n, p["n_bases"], db.bases2, db.seg1_offset, db.seg1_length, db.mean_quality, db.compression)
    nwords = e * gr.desc.hash_funs * gr.desc.bin_words
    partial = api.device_malloc(0, max(nwords, 2) * 8)
    st.shard_probe(gr, partial, nwords)
    st.shard_finish(partial)
    line("dense sharded chain", dbt.wait_downloaded(api, st, n))
    api.device_free(0, partial)
    st.destroy()
    db.free()

    # the sparse row-sharded chain: one rank, three owners (tests/test_gpu_parity.py)
    S, Wd, words = rows.bin_size, rows.bin_words, rows.words()
    splits = [0, 17, S // 3, S]
    shards = []
    for lo, hi in zip(splits[:-1], splits[1:]):
        sh = api.Index(api.make_desc(rows.bins, S, rows.bin_to_cat, 2, gr.desc.host_index, row_begin=lo, row_end=hi))
        sh.upload(words[lo * Wd:hi * Wd], row_begin=lo)
        shards.append(sh)
    st = api.Stream(shards[0], n, p["n_bases"])
    st.set_model(dbt.model_for(api, gr, False))
    st.shardx_minimise_host(p, *dbt.host_columns(n))
    n_probes, counts = st.shardx_counts(splits)
    dq = api.device_malloc(0, max(n_probes, 1) * 4)
    st.shardx_queries(dq, n_probes)
    st.sync()
    back = api.device_malloc(0, max(n_probes, 1) * Wd * 8)
    at = 0
    for o, sh in enumerate(shards):  # the owners serve their groups in place: query group o is [at, at + counts[o])
        if counts[o]:
            st.shardx_serve(sh, dq + at * 4, counts[o], back + at * Wd * 8)
        at += counts[o]
    st.sync()
    st.shardx_finish(back)
    line("sparse sharded chain", st.wait_host())
    for ptr in (dq, back):
        api.device_free(0, ptr)
    st.destroy()
    for sh in shards:
        sh.destroy()

    # W = 1 .. 4 words per row, row-log layout, device-made reads
    glen, nr = 1 << 14, 4096
    for B in (40, 100, 130, 200):
        g = api.Index(api.make_desc(B, 1 << 18, [b % 2 for b in range(B)], 2, 0))
        gen = api.synth_genomes(0, 43, B, glen)
        g.synth_fill(43, 0.1)
        g.synth_plant(gen, B, glen, list(range(B)))
        rd = api.synth_reads(0, 45, gen, B, glen, nr, 200, 400, 0.05, 0.1, 40.0)
        st = api.Stream(g, nr, int(rd.n_bases))
        st.set_model(api.default_model(2, 0))
        for _ in range(3):
            st.submit_device(nr, rd.n_bases, rd.bases2, rd.seg1_offset, rd.seg1_length, rd.mean_quality, rd.compression)
        for k in range(3):
            line("W = %d, %d bins, device batch %d of 3" % (g.desc.bin_words, B, k + 1), util.download_results(api, st.wait_device(), nr, 2))
        st.destroy()
        util.free_synth_reads(api, rd)
        api.device_free(0, gen)
        g.destroy()

    for x in (gf, gr, gse):
        x.destroy()
    for x in (fused, rows, fused_se):
        x.free()
    print("done")


if __name__ == "__main__":
    main()
