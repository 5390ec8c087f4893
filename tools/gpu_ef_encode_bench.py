#!/usr/bin/env python3
"""chn_index_encode_ef alone: a synthetic index (chn_synth_fill_index) of some size at some densities -- device_ms (the kernels, from
events), the whole call (host clock; the call is synchronous), and beside it two chn_index_download_rows passes over the same index, which
is what the host path of `charon index` moves before its threads start on the bits.  GB/s are of PLAIN index.
usage: python tools/gpu_ef_encode_bench.py [MiB of index = 1024] [densities = 0.05,0.3] [repeats = 3]"""
import os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charon_amd.api as api

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
densities = [float(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "0.05,0.3").split(",")]
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
rows = mib * (1 << 20) // 8  # 64 bins: one word a row
gb = rows * 8 / 1e9
spread = lambda v: "%.1f - %.1f - %.1f" % (min(v), statistics.median(v), max(v))
for density in densities:
    g = api.Index(api.make_desc(64, rows, [0] * 64, 1, 0))
    g.synth_fill(7, density)
    lay = g.ef_layout()
    job, low, high = api.ef_encode_job(lay)
    dev, call, down = [], [], []
    block_rows = (256 << 20) // 8
    block = np.zeros(min(rows, block_rows), np.uint64)
    for rep in range(repeats + 1):  # the first round warms up (code objects, page-locked staging, first touch of the arrays)
        t0 = time.perf_counter()
        api._chk(api.lib().chn_index_encode_ef(g.h, api.C.byref(job)))
        t1 = time.perf_counter()
        for _ in range(2):
            for r0 in range(0, rows, block_rows):
                nr = min(block_rows, rows - r0)
                api._chk(api.lib().chn_index_download_rows(g.h, r0, nr, block.ctypes.data))
        t2 = time.perf_counter()
        if rep:
            dev.append(job.device_ms); call.append((t1 - t0) * 1e3); down.append((t2 - t1) * 1e3)
    assert job.ones_written == lay.ones
    print("index %.2f GB, density %.3f: %d set bits, wl %d, m_low %.1f MB, m_high %.1f MB" % (gb, density, lay.ones, lay.wl, lay.n_low_words * 8 / 1e6, lay.n_high_words * 8 / 1e6))
    print("  device_ms            %s ms   (%.1f GB/s of plain index at the median)" % (spread(dev), gb / statistics.median(dev) * 1e3))
    print("  whole call           %s ms   (%.2f GB/s)" % (spread(call), gb / statistics.median(call) * 1e3))
    print("  two download passes  %s ms   (%.2f GB/s of plain index, each byte moved twice)" % (spread(down), gb / statistics.median(down) * 1e3), flush=True)
    g.destroy()
