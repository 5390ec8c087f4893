"""Shared helpers for the parity tests: seeded synthetic genomes/reads and oracle<->GPU index mirroring."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rng(seed):
    return np.random.default_rng(seed)


def random_seq(r, n):
    return np.frombuffer(b"ACGT", np.uint8)[r.integers(0, 4, n)].tobytes()


def mutate(r, seq, rate):
    a = np.frombuffer(seq, np.uint8).copy()
    hit = r.random(a.size) < rate
    alt = np.frombuffer(b"ACGT", np.uint8)[r.integers(0, 4, a.size)]
    a[hit] = alt[hit]
    return a.tobytes()


def sample_reads(r, genomes, n, length, sub_rate=0.05, random_fraction=0.1):
    """genomes: list of bytes.  Returns list of reads (bytes)."""
    out = []
    for _ in range(n):
        L = int(length if np.isscalar(length) else r.integers(length[0], length[1] + 1))
        if r.random() < random_fraction or not genomes:
            out.append(random_seq(r, L))
        else:
            g = genomes[int(r.integers(0, len(genomes)))]
            if len(g) <= L:
                out.append(mutate(r, g, sub_rate))
            else:
                s = int(r.integers(0, len(g) - L))
                out.append(mutate(r, g[s:s + L], sub_rate))
    return out


def build_oracle_index(po, genomes_by_bin, bin_to_cat, categories, k=19, w=41, bin_size=None, fill_seed=None, fill=0.0, hash_funs=3):
    """genomes_by_bin: list (one entry per bin) of lists of sequences.  Inserts the distinct minimisers of every
    sequence into its bin (what `charon index` does, src/index_main.cpp:118-160,238-263)."""
    mins = []
    for seqs in genomes_by_bin:
        s = set()
        for g in seqs:
            s.update(int(x) for x in po.minimisers(g.decode() if isinstance(g, bytes) else g, k, w))
        mins.append(np.array(sorted(s), dtype=np.uint64))
    if bin_size is None:
        bin_size = int(po.lib().orc_bin_size_in_bits(max(1, max(len(m) for m in mins)), hash_funs, 0.01))
    idx = po.Index.new(len(genomes_by_bin), bin_size, bin_to_cat, categories, k=k, w=w, nhash=hash_funs)
    if fill_seed is not None and fill > 0:
        r = rng(fill_seed)
        words = idx.words()
        B = len(genomes_by_bin)
        for wd in range(idx.bin_words):
            nb = min(64, B - 64 * wd)
            if nb <= 0:
                continue
            bits = (r.random((idx.bin_size, nb)) < fill)
            vals = np.zeros(idx.bin_size, np.uint64)
            for b in range(nb):
                vals |= bits[:, b].astype(np.uint64) << np.uint64(b)
            words[wd::idx.bin_words] |= vals
    for b, m in enumerate(mins):
        if len(m):
            idx.emplace_many(m, b)
    return idx


def gpu_index_from_oracle(api, oidx, device=0):
    host = oidx.host_index if oidx.host_index < 255 else 255
    desc = api.make_desc(oidx.bins, oidx.bin_size, oidx.bin_to_cat, oidx.ncat, host, k=oidx.k, w=oidx.w,
                         hash_funs=oidx.hash_funs, device=device)
    g = api.Index(desc)
    g.upload(oidx.words())
    return g


def concat(reads, mates=None):
    """-> (bytes, offsets uint64[n+1], mate_split or None) in the oracle's input layout"""
    parts, offs, split = [], [0], []
    for i, s in enumerate(reads):
        t = s + (mates[i] if mates is not None else b"")
        parts.append(t)
        offs.append(offs[-1] + len(t))
        split.append(len(s))
    return b"".join(parts), np.array(offs, np.uint64), (np.array(split, np.uint32) if mates is not None else None)


def assert_parity(gpu, orc, prob_tol=1e-6):
    """bit-exact integer columns; probability column within the north-star tolerance (1e-6)."""
    np.testing.assert_array_equal(gpu["num_hashes"], orc["num_hashes"])
    np.testing.assert_array_equal(gpu["counts"], orc["counts"])
    np.testing.assert_array_equal(gpu["unique"], orc["unique"])
    np.testing.assert_array_equal(gpu["conf"], orc["conf"])
    np.testing.assert_array_equal(gpu["call"], orc["call"])
    a, b = gpu["probs"], orc["probs"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert np.max(np.abs(a[ok] - b[ok]), initial=0.0) <= prob_tol


def download_results(api, res, n, ncat, device=0, gzip_output=None):
    """device-resident chn_result -> the dict layout of Stream.wait_host().  gzip_output: what the batch asked for (its
    chn_batch.gzip_output; None: no gzip column) -- the columns the result carries for it come back as gzip_sizes and gzip_tallies
    ([n][320] uint16; with device results the tallies' status word is there in every mode)"""
    out = dict(num_hashes=api.device_download(device, res.num_hashes, n * 4, np.uint32),
               counts=api.device_download(device, res.counts, n * ncat * 4, np.uint32).reshape(n, ncat),
               unique=api.device_download(device, res.unique_counts, n * ncat * 4, np.uint32).reshape(n, ncat),
               probs=api.device_download(device, res.probabilities, n * ncat * 8, np.float64).reshape(n, ncat),
               call=api.device_download(device, res.call, n, np.uint8), conf=api.device_download(device, res.confidence, n, np.uint8),
               flags=api.device_download(device, res.flags, n, np.uint8))
    if gzip_output is not None:
        if res.gzip_sizes:
            out["gzip_sizes"] = api.device_download(device, res.gzip_sizes, n * 4, np.uint32)
        if res.gzip_tallies:
            out["gzip_tallies"] = api.device_download(device, res.gzip_tallies, n * 320 * 2, np.uint16).reshape(n, 320)
    return out


def to_device(api, arr, device=0):
    """a device buffer holding `arr` (at least 16 bytes); the caller frees it with api.device_free"""
    arr = np.ascontiguousarray(arr)
    p = api.device_malloc(device, max(arr.nbytes, 16))
    if arr.nbytes:
        api.device_upload(device, p, arr)
    return p


class DeviceBatch:
    """what pack.pack_reads returns, in device buffers of its own: the pointers of a chn_batch with on_device = 1"""
    POINTERS = ("bases2", "nmask", "seg1_offset", "seg1_length", "seg2_offset", "seg2_length", "mean_quality", "compression")

    def __init__(self, api, packed, mq=None, comp=None, device=0):
        self.api, self.device = api, device
        self.n_reads, self.n_bases = len(packed["seg1_length"]), int(packed["n_bases"])
        col = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (self.n_reads,)))
        host = dict(bases2=(packed["bases2"], np.uint32), nmask=(packed.get("nmask"), np.uint32),
                    seg1_offset=(packed["seg1_offset"], np.uint64), seg1_length=(packed["seg1_length"], np.uint32),
                    seg2_offset=(packed.get("seg2_offset"), np.uint64), seg2_length=(packed.get("seg2_length"), np.uint32),
                    mean_quality=(col(mq), np.float32), compression=(col(comp), np.float32))
        for key, (a, dt) in host.items():
            setattr(self, key, None if a is None else to_device(api, np.ascontiguousarray(a, dtype=dt), device))

    def submit(self, st, gzip_tallies=0, gzip_output=0, **other):
        """chn_batch_submit of this batch on stream `st`; other: pointers to use instead of the batch's own (nmask=None, ...)"""
        p = {key: other.get(key, getattr(self, key)) for key in self.POINTERS}
        st.submit_device(self.n_reads, self.n_bases, p["bases2"], p["seg1_offset"], p["seg1_length"], p["mean_quality"], p["compression"],
                         nmask=p["nmask"], seg2_offset=p["seg2_offset"], seg2_length=p["seg2_length"], gzip_tallies=gzip_tallies,
                         gzip_output=gzip_output)

    def free(self):
        for key in self.POINTERS:
            self.api.device_free(self.device, getattr(self, key))
            setattr(self, key, None)


def to_device_batch(api, packed, mq=None, comp=None, device=0):
    """upload a packed batch (bases2, nmask if present, seg1_*, seg2_* if present, the two float columns -- scalars or arrays, None:
    no column) -> DeviceBatch"""
    return DeviceBatch(api, packed, mq, comp, device)


def free_synth_reads(api, rd, device=0):
    for p in (rd.bases2, rd.seg1_offset, rd.seg1_length, rd.mean_quality, rd.compression):
        api.device_free(device, p)


def assert_same_results(a, b, keys=("num_hashes", "counts", "unique", "call", "conf", "probs")):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True) if key == "probs" else np.array_equal(a[key], b[key]), key


def kde_tables(seed=71):
    """synthetic KDE datasets of the model tests (tests/test_model_ref_cpu.py, tests/test_gpu_model_call.py), in the order the
    kernel must iterate them: name -> float32 array.  'trained' is unsorted with values of many magnitudes, so its float sum
    depends on the order of the terms."""
    r = rng(seed)
    t = {"n0": np.zeros(0, np.float32), "n1": np.float32([0.05])}
    t["n63_dup"] = np.sort(np.round(r.uniform(0.0, 0.3, 63), 2)).astype(np.float32)  # many duplicates
    v = r.uniform(0.0, 1.0, 64).astype(np.float32)
    v[[5, 40]] = np.inf
    v[17] = -np.inf
    t["n64_inf"] = v
    v = r.uniform(0.0, 0.2, 65).astype(np.float32)
    v[31] = np.nan
    t["n65_nan"] = v
    t["trained"] = np.concatenate([r.lognormal(-3.0, 1.5, 600), r.uniform(0.0, 0.02, 400)]).astype(np.float32)
    r.shuffle(t["trained"])
    t["n4097"] = r.beta(2.0, 12.0, 4097).astype(np.float32)
    return t
