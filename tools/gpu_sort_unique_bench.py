#!/usr/bin/env python3
"""chn_hashset_unique alone: the radix sort and unique pass over n keys already in device memory (the upload is not timed), the whole call by
the host clock (it is synchronous: its allocations, the histogram's trip to the host and the count's are inside).  Two kinds of keys:
random 64-bit ones (8 passes run), and keys whose two top bytes are constants, as the minimisers of k = 19 are (6 passes run).  Beside
it, once, numpy.unique of the same keys on the host: a scale, not a target.
usage: python tools/gpu_sort_unique_bench.py [log2 n, comma list = 26,28] [repeats = 3]"""
import os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import charon_amd.api as api

logs = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "26,28").split(",")]
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
spread = lambda v: "%.1f - %.1f - %.1f" % (min(v), statistics.median(v), max(v))
r = np.random.default_rng(11)
for lg in logs:
    n = 1 << lg
    for kind in ("random", "two constant bytes"):
        keys = r.integers(0, 2 ** 64 - 1, n, dtype=np.uint64, endpoint=True)
        if kind != "random":
            keys = (keys >> np.uint64(16)) ^ np.uint64(0x8F3F73B5CF1C9ADE & ~0xFFFFFFFFFFFF)
        # the passes that run: those whose byte is not the same in every key
        ran = [j for j in range(8) if np.ptp((keys >> np.uint64(8 * j)).astype(np.uint8)) != 0]
        ms, distinct = [], 0
        for rep in range(repeats + 1):  # the first round warms up (code objects, the allocator) and is discarded
            hs = api.HashSet()
            hs.append(keys)
            t0 = time.perf_counter()
            distinct = hs.unique()
            t1 = time.perf_counter()
            if rep:
                ms.append((t1 - t0) * 1e3)
            if rep == repeats:
                first, last = hs.download(0, 1)[0], hs.download(distinct - 1, 1)[0]
            hs.destroy()
        t0 = time.perf_counter()
        want = np.unique(keys)
        host_ms = (time.perf_counter() - t0) * 1e3
        ok = want.size == distinct and want[0] == first and want[-1] == last
        print("2^%d keys, %s: passes %s ran, %d distinct%s" % (lg, kind, ran, distinct, "" if ok else "  -- DIFFERS from numpy.unique (%d)" % want.size))
        print("  chn_hashset_unique  %s ms   (%.2f G keys/s at the median)   [min - median - max of %d]" % (spread(ms), n / statistics.median(ms) / 1e6, repeats))
        print("  numpy.unique        %.0f ms   (%.3f G keys/s; one run, one host thread)" % (host_ms, n / host_ms / 1e6), flush=True)
        if not ok:
            sys.exit(1)
