#!/usr/bin/env python3
"""Rate of chn_index_replicate (one hipMemcpyPeerAsync of the index words) onto the SAME device, on a synthetic index.

usage: python tools/replicate_rate.py [GiB of index words, default 8] [repeats, default 3]
The source is filled at 10 % density (chn_synth_fill_index); every replica's set bits per bin are checked against the source's.
Prints one line per repeat (seconds from the call to the end of the copy, GB/s of words copied) and a JSON summary line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    gib = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    import numpy as np
    import charon_amd.api as api
    bins = 64  # one word per row
    rows = int(gib * (1 << 30)) // 8
    desc = api.make_desc(bins, rows, [i % 2 for i in range(bins)], 2, 1, device=0)
    src = api.Index(desc)
    src.synth_fill(7, 0.1)
    want = src.bin_popcounts()
    nbytes = rows * 8
    rates = []
    for i in range(reps):
        t0 = time.perf_counter()
        rep = src.replicate(0)
        t_queued = time.perf_counter() - t0
        rep.download(0, 1)  # waits for the copy
        dt = time.perf_counter() - t0
        ok = bool(np.array_equal(rep.bin_popcounts(), want))
        rep.destroy()
        rates.append(nbytes / dt / 1e9)
        print("replicate %.2f GB on device 0: queued in %.4f s, copied in %.4f s -> %.1f GB/s, popcounts equal: %s"
              % (nbytes / 1e9, t_queued, dt, rates[-1], ok), flush=True)
        if not ok:
            sys.exit(1)
    src.destroy()
    print(json.dumps({"metric": "chn_index_replicate, same device", "bytes": nbytes, "gb_per_s": rates, "best_gb_per_s": max(rates)}))


if __name__ == "__main__":
    main()
