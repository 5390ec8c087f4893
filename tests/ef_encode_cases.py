"""Cases of the Elias-Fano encode (chn_index_encode_ef, chn_index_encode_ef_host), shared by tests/test_ef_encode_cpu.py and
tests/test_gpu_ef_encode.py: the smallest shapes at which the rule, the slices' seams or the kernel's scan can go wrong.

A case is (name, bins, bin_size, maker, slices): maker(rng, bins, tb, bin_size) returns the ascending plain positions
pos = row * technical_bins + bin of the set bits; `slices` are the slice_rows values the case runs with.  Positions come from a generator
seeded by the case's name.  The expected arrays are oracle.pyref.ef_encode of the positions (the independent restatement of sdsl's sd_vector
layout), computed once per case and shared.

LARGE / build_large are the shapes with thousands of blocks a slice (tests/test_gpu_ef_scale.py and the host form's CPU test): their expected
arrays are ef_encode_np's, the numpy restatement of pyref.ef_encode.  SEAM is one more small case, for the decode's slice seams."""
import functools
import zlib

import numpy as np

from oracle import pyref


def _random(ones, all_bins=False):
    def make(rng, bins, tb, bin_size):
        rows = rng.integers(0, bin_size, ones * 2)
        cols = rng.integers(0, tb if all_bins else bins, ones * 2)
        return np.unique(rows.astype(np.int64) * tb + cols)[:ones]
    return make


def _all_real_bits(rng, bins, tb, bin_size):
    return (np.arange(bin_size, dtype=np.int64)[:, None] * tb + np.arange(bins, dtype=np.int64)[None, :]).ravel()


def _fixed(positions):
    return lambda rng, bins, tb, bin_size: np.array([p if p >= 0 else tb * bin_size + p for p in positions], np.int64)


def _in_rows(rows_and_counts):
    """`count` random bits in each of the given rows, nothing elsewhere"""
    def make(rng, bins, tb, bin_size):
        out = []
        for row, count in rows_and_counts:
            out.append(row * tb + np.sort(rng.choice(bins, count, replace=False)).astype(np.int64))
        return np.concatenate(out)
    return make


def _technical_only(rng, bins, tb, bin_size):
    """bits in the technical-only bins (>= bins) of a third of the rows, some real ones beside them"""
    rows = rng.integers(0, bin_size, 400)
    cols = np.where(rng.random(400) < 0.7, rng.integers(bins, tb, 400), rng.integers(0, bins, 400))
    return np.unique(rows.astype(np.int64) * tb + cols)


def _blocks_of_256(rng, bins, tb, bin_size):
    """one word a row: words 0..255 all ones, 256..511 all zeros, 512..767 all ones, 768..1023 zeros, then noise"""
    w = np.zeros(bin_size, np.uint64)
    w[0:256] = ~np.uint64(0)
    w[512:768] = ~np.uint64(0)
    w[1024:] = rng.integers(0, 2 ** 63, bin_size - 1024, dtype=np.uint64) & rng.integers(0, 2 ** 63, bin_size - 1024, dtype=np.uint64)
    return np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")).astype(np.int64)


def _three_ways(given, bin_size):
    return (given, 1, bin_size)


CASES = [
    # the five shapes of test_device_elias_fano_decode, each with the given slice, with one row a slice and as one slice
    ("decode_100x5000", 100, 5000, _random(60000), _three_ways(64, 5000)),
    ("decode_8x70001", 8, 70001, _random(300000), _three_ways(1000, 70001)),
    ("decode_130x997_one", 130, 997, _random(1), _three_ways(1 << 20, 997)),
    ("decode_3x4096_full", 3, 4096, _all_real_bits, _three_ways(7, 4096)),
    ("decode_200x3001", 200, 3001, _random(150000), _three_ways(33, 3001)),
    ("empty", 5, 100, _fixed([]), (0, 7)),
    ("bit_at_0", 64, 50, _fixed([0]), (0, 1, 7)),
    ("bit_at_last", 64, 50, _fixed([-1]), (0, 1, 7)),
    ("full_64x64", 64, 64, _all_real_bits, (0, 1, 5)),            # logm == logn: the decrement applies
    ("ones_2j_minus_1", 64, 100, _random(255), (0, 9)),          # wl changes between 255 and 256 ones
    ("ones_2j", 64, 100, _random(256), (0, 9)),
    ("ones_2j_plus_1", 64, 100, _random(257), (0, 9)),
    ("straddle", 64, 1000, _random(100), (0, 1, 13)),             # wl = 9: low elements straddle words
    ("one_bin_2_20_rows", 1, 1 << 20, _fixed([5 * 64, (1 << 19) * 64, -64]), (0, 1 << 18)),   # wl = 25, long zero runs in m_high
    ("technical_only_bins", 3, 300, _technical_only, (0, 1, 11)),
    # slice boundaries (8 rows a slice) directly behind / in front of the one row that holds all of a slice's ones
    ("ones_at_slice_edges", 130, 40, _in_rows([(7, 90), (8, 120), (23, 64), (24, 1), (39, 130)]), (8, 0)),
    ("empty_slice_between", 100, 30, _in_rows([(r, 40) for r in range(0, 10)] + [(r, 55) for r in range(20, 30)]), (10, 0)),
    ("blocks_of_256", 64, 1500, _blocks_of_256, (0, 300, 256)),
]
CASE = {c[0]: c for c in CASES}
RUNS = [(c[0], s) for c in CASES for s in c[4]]


def to_words(value, bits):
    """python int (bit i = position i) -> numpy uint64 words"""
    return np.frombuffer(int(value).to_bytes(((bits + 63) // 64) * 8, "little"), np.uint64).copy()


@functools.lru_cache(maxsize=None)
def build(name):
    """the case's data: bins, bin_size, tb, universe, pos, words (plain rows), and the expected wl, low_bits, low, high_bits, high"""
    _, bins, bin_size, maker, _ = CASE[name]
    tb = (bins + 63) // 64 * 64
    universe = tb * bin_size
    pos = np.asarray(maker(np.random.default_rng(zlib.crc32(name.encode())), bins, tb, bin_size), np.int64)
    assert (np.diff(pos) > 0).all() and (pos.size == 0 or (pos[0] >= 0 and pos[-1] < universe))
    words = np.zeros(universe // 64, np.uint64)
    np.bitwise_or.at(words, pos >> 6, np.uint64(1) << (pos & 63).astype(np.uint64))
    wl, low_bits, low, high_bits, high = pyref.ef_encode([int(p) for p in pos], universe)
    d = dict(name=name, bins=bins, bin_size=bin_size, tb=tb, universe=universe, pos=pos, words=words, wl=wl, low_bits=low_bits,
             low=to_words(low, low_bits), high_bits=high_bits, high=to_words(high, high_bits))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def ef_encode_np(pos, universe):
    """oracle.pyref.ef_encode in numpy, for position lists pyref's Python integers cannot carry: (wl, low_bits, low_words, high_bits,
    high_words) with both arrays as uint64 words.  The same rule, restated: logm = hi(m) + 1, logn = hi(universe) + 1, logm one less where
    they are equal; wl = logn - logm; the one of rank k at position p has bit (p >> wl) + k of m_high and p's low wl bits at bit k * wl of
    m_low.  Built from bit planes and np.packbits, a byte a bit, so it shares nothing with the kernels' word arithmetic; test_ef_encode_cpu
    pins it to pyref on every case of CASES."""
    pos = np.asarray(pos, np.uint64)
    m = int(pos.size)
    hi = lambda x: x.bit_length() - 1 if x else 0
    logm, logn = hi(m) + 1, hi(int(universe)) + 1
    if logm == logn:
        logm -= 1
    wl = logn - logm
    low_bits, high_bits = m * wl, m + (1 << logm)

    def packed(bits, n_bits):
        out = np.zeros((n_bits + 63) // 64 * 8, np.uint8)
        b = np.packbits(bits, bitorder="little")
        out[:b.size] = b
        return out.view(np.uint64)

    planes = np.empty((m, wl), np.uint8)
    for j in range(wl):
        planes[:, j] = (pos >> np.uint64(j)) & np.uint64(1)
    high = np.zeros(high_bits, np.uint8)
    high[(pos >> np.uint64(wl)) + np.arange(m, dtype=np.uint64)] = 1
    return wl, low_bits, packed(planes.ravel(), low_bits), high_bits, packed(high, high_bits)


def positions_of(words):
    """ascending bit numbers of the set bits of uint64 words (bit i of word w is position 64 * w + i), a piece at a time"""
    step = 1 << 20
    out = [np.flatnonzero(np.unpackbits(words[i:i + step].view(np.uint8), bitorder="little")) + i * 64 for i in range(0, words.size, step)]
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)


_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)  # set bits of a byte
PREFIX_CHUNK = 1024  # block counts k_ef_block_prefix takes a round (array_scan, parts/scan.inc: 256 threads, four counts each); the sum so far is carried in a register
BLOCK_WORDS = 256    # words whose ones k_ef_block_counts adds up into one count


def block_counts(words):
    """set bits per block of 256 words, as k_ef_block_counts counts them (the last block may be short)"""
    per_word = _POP8[words.view(np.uint8)].reshape(-1, 8).sum(axis=1, dtype=np.int64)
    return np.add.reduceat(per_word, np.arange(0, per_word.size, BLOCK_WORDS))


def prefix_chunks(n_words):
    """rounds of 1024 counts that k_ef_block_prefix's scan takes for the blocks of n_words words"""
    n_blocks = (n_words + BLOCK_WORDS - 1) // BLOCK_WORDS
    return (n_blocks + PREFIX_CHUNK - 1) // PREFIX_CHUNK


def uneven_in_every_chunk(words, slice_words):
    """the block counts of every slice of `slice_words` words differ within every chunk the prefix kernel takes (a chunk of one count aside)"""
    for w0 in range(0, words.size, slice_words):
        counts = block_counts(words[w0:w0 + slice_words])
        for c in range(0, counts.size, PREFIX_CHUNK):
            chunk = counts[c:c + PREFIX_CHUNK]
            if chunk.size > 1 and (chunk == chunk[0]).all():
                return False
    return True


def _random_words(rng, n, ands, ors=0):
    """n words of the AND of `ands` random words and of the OR of `ors` more: a bit is set with probability 2^-ands * (1 - 2^-ors)"""
    r = lambda: rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    w = r()
    for _ in range(ands - 1):
        w &= r()
    if ors:
        o = r()
        for _ in range(ors - 1):
            o |= r()
        w &= o
    return w


# Shapes whose slices have thousands of 256-word blocks, so that k_ef_block_prefix's scan takes several rounds of 1024 counts and carries from one to the next.  64 bins, one word a
# row.  They are kept apart from CASES: oracle.pyref is never asked for them; the expected arrays are ef_encode_np's.
#
# many_blocks: one bit in eight, ~2^24 + 2.6e5 ones in 2^27.02 bits: logm = 25, logn = 28, wl = 3.  m_high has ~790 000 words = ~3090
# blocks: 4 rounds of the loop for a decode of it in one slice.  The plain index has 8320 blocks: 9 rounds for an encode in one slice.
# 16.25 MiB.
#
# many_blocks_thin: the thin one, with low elements that straddle words.  Two rounds on the decode need high_bits = m + 2^logm > 2^24, so
# logm >= 24 and m >= 2^23 ones; an index below 32 MiB has logn <= 28, so wl <= 4, and of those only 3 does not divide 64 -- which takes
# many_blocks' density.  So this case is the smallest that does meet both: 2^22 + 2^15 rows (32.25 MiB, logn = 29) with three bits in 64,
# ~1.26e7 ones: logm = 24, wl = 5.  m_high has ~459 000 words = ~1790 blocks: 2 rounds on the decode, 17 on a one-slice encode.  (A wl of 7
# with two rounds needs logn = 31: 128 MiB.)  A plain block holds ~770 ones where many_blocks has ~2050.
LARGE = {
    "many_blocks": dict(bin_size=(1 << 21) + (1 << 15), ands=3, ors=0, decode_rounds=3, straddles=False, max_bytes=32 << 20),
    "many_blocks_thin": dict(bin_size=(1 << 22) + (1 << 15), ands=4, ors=2, decode_rounds=2, straddles=True, max_bytes=33 << 20),
}
LARGE_SLICE_ROWS = (1 << 18) + 1  # 1025 blocks a slice: one block into the second round


@functools.lru_cache(maxsize=None)
def build_large(name):
    """as build(), from ef_encode_np; `per_bin` are the set bits per bin"""
    spec = LARGE[name]
    bins = tb = 64
    bin_size = spec["bin_size"]
    universe = tb * bin_size
    words = _random_words(np.random.default_rng(zlib.crc32(name.encode())), bin_size, spec["ands"], spec["ors"])
    pos = positions_of(words)
    wl, low_bits, low, high_bits, high = ef_encode_np(pos, universe)
    # a decode of the whole m_high in one slice goes round the prefix loop this often: the carry is added to (rounds - 1) times
    assert high.size > (spec["decode_rounds"] - 1) * PREFIX_CHUNK * BLOCK_WORDS and prefix_chunks(high.size) >= spec["decode_rounds"]
    assert words.size > 2048 * BLOCK_WORDS  # and an encode of the whole index in one slice at least three times
    # (m_high ends in zeros -- the universe is well below 2^logn, so the last high parts are never reached: the rounds are counted and
    # the counts looked at up to the last one)
    used = high[:np.flatnonzero(high)[-1] + 1]
    assert prefix_chunks(used.size) >= spec["decode_rounds"]
    assert uneven_in_every_chunk(used, used.size) and uneven_in_every_chunk(used, PREFIX_CHUNK * BLOCK_WORDS + 1)
    assert uneven_in_every_chunk(words, words.size) and uneven_in_every_chunk(words, LARGE_SLICE_ROWS)
    assert words.size * 8 < spec["max_bytes"]
    if spec["straddles"]:
        assert 64 % wl != 0
    d = dict(name=name, bins=bins, bin_size=bin_size, tb=tb, universe=universe, pos=pos, words=words, wl=wl, low_bits=low_bits, low=low,
             high_bits=high_bits, high=high, per_bin=np.bincount(pos % tb, minlength=tb).astype(np.uint64))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# wl = 10 (low elements straddle words) with an m_high of ~207 words: decode slices of a few words begin at ranks that are no multiple of
# 64, in the middle of a word of m_low.  build() knows the case; CASES and RUNS (the encode's runs) stay as they are.
SEAM = ("straddle_many_slices", 64, 100000, _random(5000), (0,))
CASE[SEAM[0]] = SEAM


def real_words(case):
    """the rows the decode leaves: the case's words without the bits in technical-only bins (which it counts as ill-placed), and their number"""
    tb, bins = case["tb"], case["bins"]
    real = case["pos"][case["pos"] % tb < bins]
    want = np.zeros(case["universe"] // 64, np.uint64)
    np.bitwise_or.at(want, real >> 6, np.uint64(1) << (real & 63).astype(np.uint64))
    return want, case["pos"].size - real.size


def assert_is_expected(case, layout, low, high):
    """wl, the bit counts and both arrays, word for word, against oracle.pyref.ef_encode of the case's positions"""
    assert (layout.wl, layout.m_size, layout.ones) == (case["wl"], case["universe"], case["pos"].size)
    assert (layout.low_bits, layout.high_bits) == (case["low_bits"], case["high_bits"])
    assert (layout.n_low_words, layout.n_high_words) == (case["low"].size, case["high"].size)
    assert np.array_equal(low, case["low"]), np.flatnonzero(low != case["low"])[:8]
    assert np.array_equal(high, case["high"]), np.flatnonzero(high != case["high"])[:8]
