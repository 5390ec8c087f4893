"""The member set of the inflate tests (tests/test_inflate_cpu.py, tests/test_gpu_inflate.py): small raw deflate members made with
Python's zlib or a bit writer, and the yardstick that says which of them a decoder must accept -- Python's zlib, never the code under
test.  Everything is seeded, so both test files see the same bytes.  crafted_set / crafted_sweep / foreign_set further down are the
members zlib's deflate never writes: made with tests/deflate_writer.py, or by libdeflate (tests/golden/foreign_members.bin)."""
import functools
import random
import zlib

MAX_OUT = 65536


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush_mode=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for f in flush_at:
        out += c.compress(data[at:f]) + c.flush(flush_mode)
        at = f
    return out + c.compress(data[at:]) + c.flush()


def yardstick(data, size):
    """(accept, bytes): what zlib's inflate makes of `data` when exactly `size` bytes are expected"""
    try:
        o = zlib.decompressobj(-15)
        out = o.decompress(data, size + 1)
    except zlib.error:
        return False, None
    ok = o.eof and len(out) == size
    return ok, (out if ok else None)


def btype(data):
    return (data[0] >> 1) & 3


def fastq_text(n, seed):
    r = random.Random(seed)
    out, i = bytearray(), 0
    while len(out) < n:
        length = r.randint(120, 400)
        out += b"@read_%d len=%d\n" % (i, length) + bytes(r.choice(b"ACGT") for _ in range(length)) + b"\n+\n"
        out += bytes(r.choice(b"FFFFFFFF:,#") for _ in range(length)) + b"\n"
        i += 1
    return bytes(out[:n])


class BitWriter:
    """deflate's bit order: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.bits = []

    def field(self, value, n):
        self.bits += [(value >> i) & 1 for i in range(n)]

    def code(self, value, n):
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def far_match(length_symbol, length_extra, dist_extra):
    """a non-final stored block of 32 768 bytes, then a final fixed block: one match with distance code 29, end of block"""
    r = random.Random(77)
    first = bytes(r.randrange(256) for _ in range(32768))
    w = BitWriter()
    w.field(1, 1); w.field(1, 2)                        # BFINAL, fixed Huffman
    w.code(0xC0 + (length_symbol - 280), 8)             # length symbols 280 .. 287 are the 8-bit codes 11000000 ..
    w.field(length_extra, {284: 5, 285: 0}[length_symbol])
    w.code(29, 5); w.field(dist_extra, 13)
    w.code(0, 7)                                        # end of block
    data = b"\x00\x00\x80\xff\x7f" + first + w.bytes()
    length = {284: 227, 285: 258}[length_symbol] + length_extra
    dist = 24577 + dist_extra
    text = bytearray(first)
    for _ in range(length):
        text.append(text[-dist])
    return data, bytes(text)


def oversubscribed_code_length_code():
    w = BitWriter()
    w.field(1, 1); w.field(2, 2)                        # BFINAL, dynamic Huffman
    w.field(0, 5); w.field(0, 5); w.field(15, 4)        # HLIT 257, HDIST 1, HCLEN 19
    for _ in range(19):
        w.field(1, 3)                                   # nineteen 1-bit codes
    w.field(0, 32)
    return w.bytes()


@functools.lru_cache(maxsize=None)
def member_set():
    """list of (name, data, size): the good members first, then the ones that must be rejected, then the one with trailing bytes"""
    r = random.Random(2024)
    text = fastq_text(65280, 1)
    rnd = bytes(r.randrange(256) for _ in range(MAX_OUT))
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    deep = bytearray()
    for v, f in enumerate(fib):
        deep += bytes([40 + v]) * f
    r.shuffle(deep)
    deep = bytes(deep[:MAX_OUT])
    dyn = raw(text)
    far1, far1_text = far_match(285, 0, 8191)
    far2, far2_text = far_match(284, 31, 0)
    good = [
        ("stored", raw(text, 0), len(text)),
        ("fixed", raw(text, 6, zlib.Z_FIXED), len(text)),
        ("fixed_one_byte", raw(b"A"), 1),
        ("dynamic", dyn, len(text)),
        ("empty", raw(b""), 0),
        ("random_max", raw(rnd), MAX_OUT),
        ("run_of_a", raw(b"A" * MAX_OUT), MAX_OUT),
        ("huffman_only", raw(text, 6, zlib.Z_HUFFMAN_ONLY), len(text)),
        ("rle", raw(text, 6, zlib.Z_RLE), len(text)),
        ("sync_flush", raw(text, 6, flush_at=(1000, 30000)), len(text)),
        ("full_flush", raw(text, 6, flush_at=(1000, 30000), flush_mode=zlib.Z_FULL_FLUSH), len(text)),
        ("deep_codes", raw(deep, 6, zlib.Z_HUFFMAN_ONLY), len(deep)),
        ("far_32768", far1, len(far1_text)),
        ("far_24577_len_258", far2, len(far2_text)),
    ]
    bad = [
        ("block_type_3", b"\x07", 0),
        ("stored_nlen", b"\x01\x05\x00\x00\x00hello", 5),
        ("cut_in_half", dyn[:len(dyn) // 2], len(text)),
        ("one_too_small", dyn, len(text) - 1),
        ("one_too_large", dyn, len(text) + 1),
        ("match_first", b"\x03\x02\x00", 3),
        ("hlit_31", b"\xfd" + b"\x00" * 12, 1),
        ("oversubscribed", oversubscribed_code_length_code(), 1),
    ]
    trailing = [("trailing_junk", dyn + b"\x9a\x00\xff", len(text))]
    return good, bad, trailing


def check_member_set():
    """the properties of the set that can be read off the streams; the yardstick's verdict on every member"""
    good, bad, trailing = member_set()
    d = {n: (m, s) for n, m, s in good + bad + trailing}
    assert btype(d["stored"][0]) == 0 and btype(d["fixed"][0]) == 1 and btype(d["dynamic"][0]) == 2
    assert d["fixed_one_byte"][0] == raw(b"A") and len(d["fixed_one_byte"][0]) == 3 and btype(d["fixed_one_byte"][0]) == 1
    assert d["empty"][0] == b"\x03\x00"
    assert btype(d["random_max"][0]) == 0 and len(d["random_max"][0]) > MAX_OUT
    assert len(d["run_of_a"][0]) < 200
    assert b"\x00\x00\xff\xff" in d["sync_flush"][0] and b"\x00\x00\xff\xff" in d["full_flush"][0]  # the empty stored blocks
    far1, far1_text = far_match(285, 0, 8191)
    far2, far2_text = far_match(284, 31, 0)
    assert yardstick(far1, 32768 + 258) == (True, far1_text) and far1_text[-258:] == far1_text[:258]
    assert yardstick(far2, 32768 + 258) == (True, far2_text) and far2_text[-258:] == far2_text[8191:8191 + 258]
    for n, m, s in good + trailing:
        assert yardstick(m, s)[0], n
    for n, m, s in bad:
        assert not yardstick(m, s)[0], n


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """the mutation sweep: 2 000 single-byte mutations and 500 truncations each of a dynamic member and of a member of several blocks.
    List of (data, size).  The first 200 entries are a fair mix (the GPU test runs those)."""
    r = random.Random(99)
    bases = [(raw(fastq_text(6000, 5)), 6000), (raw(fastq_text(31000, 6), 6, flush_at=(1000, 30000)), 31000)]
    assert btype(bases[0][0]) == 2
    cases = []
    for data, size in bases:
        for _ in range(2000):
            at = r.randrange(len(data)) if r.random() < 0.6 else r.randrange(min(len(data), 120))  # headers are where the checks are
            m = bytearray(data)
            m[at] ^= r.randrange(1, 256)
            cases.append((bytes(m), size))
        for _ in range(500):
            cases.append((data[:r.randrange(len(data))], size))
    r.shuffle(cases)
    return cases


@functools.lru_cache(maxsize=None)
def sweep_verdicts():
    return [yardstick(m, s) for m, s in sweep_cases()]


# ---- members zlib's deflate never writes (tests/deflate_writer.py) ----------------------------------------------------------------------
STORED_ALIGN_N = (0, 1, 2, 3, 4, 5, 7, 8, 9)
STORED_IN_N = (1023, 1024, 1025, 2047, 2048, 2049)


def _rbytes(r, n):
    return bytes(r.randrange(256) for _ in range(n))


def _all_symbols(dw):
    """a non-final stored block of 32 768 random bytes, then one dynamic block of 286 + 30 codes, most of them 14 and 15 bits long, that
    uses every one of them: the 256 literals; every distance symbol with its smallest and largest extra value; every length symbol with
    its smallest and largest extra value at distance 64, 63 and 65 (lengths over 64), L, L - 1, 2 and 1 -- in front of each such group
    66 bytes copied out of the random block, so that a copy from the wrong place shows in the bytes"""
    r = random.Random(4242)
    first = _rbytes(r, 32768)
    ll_lens = [1, 2, 3, 4, 5, 6] + [14] * 232 + [15] * 48
    dd_lens = list(range(1, 11)) + [14] * 12 + [15] * 8
    r.shuffle(ll_lens); r.shuffle(dd_lens)
    assert dw.kraft(ll_lens) == 32768 and dw.kraft(dd_lens) == 32768 and len(ll_lens) == 286 and len(dd_lens) == 30
    tokens = list(range(256))
    r.shuffle(tokens)
    at = 32768 + 256
    for d in range(30):
        for dx in sorted({0, (1 << dw.DIST_EXTRA[d]) - 1}):
            ls = 257 + r.randrange(8)
            tokens.append((dw.MATCH, ls, 0, d, dx))
            at += dw.LEN_BASE[ls - 257]
    for i in range(29):
        for lx in sorted({0, (1 << dw.LEN_EXTRA[i]) - 1}):
            length = dw.LEN_BASE[i] + lx
            tokens.append(dw.match(66, at - r.randrange(max(0, at - 32768), 32768 - 66)))
            at += 66
            dists = [64] + ([63, 65] if length > 64 else []) + [length, length - 1, 2, 1]
            for dist in sorted(set(dists), key=dists.index):
                tokens.append((dw.MATCH, 257 + i, lx) + dw.dist_token(dist))
                at += length
    tokens.append(dw.EOB)
    return [dw.stored(first), dw.dynamic(tokens, ll_lens, dd_lens)]


def _many_blocks(dw):
    """200 dynamic blocks, each with fresh random tables of 286 + 30 codes of up to 15 bits, 20 literals and one match"""
    r = random.Random(303)
    blocks, at = [], 0
    for _ in range(200):
        ll_lens, dd_lens = dw.random_complete(r, range(286), 15, 286), dw.random_complete(r, range(30), 15, 30)
        i = r.randrange(29)
        m = (dw.MATCH, 257 + i, r.randrange(1 << dw.LEN_EXTRA[i])) + dw.dist_token(r.randint(1, min(at + 20, 32768)))
        blocks.append(dw.dynamic([r.randrange(256) for _ in range(20)] + [m, dw.EOB], ll_lens, dd_lens))
        at += 20 + dw.match_length(m)
    return blocks


def _lens(n, of):
    """n code lengths, zero except for of = {symbol: length}"""
    return [of.get(s, 0) for s in range(n)]


@functools.lru_cache(maxsize=None)
def _crafted():
    """(good, bad) lists of (name, blocks): see crafted_set"""
    from tests import deflate_writer as dw
    M, S, B, EOB = dw.MATCH, dw.SYM, dw.BITS, dw.EOB
    r = random.Random(808)
    A, Bb = 65, 66
    one_ll = dw.random_complete(r, [A, Bb, 256, 257, 264, 284, 285], 15, 286)
    lit_ll = dw.random_complete(r, sorted(set(b"no distance code at all")) + [256], 15, 257)
    lit257_ll = dw.random_complete(r, [A, Bb, 256, 257], 15, 258)
    # a, 256, 257, 258 at 1, 2, 3, 3 bits and distance symbols 0 .. 5 at 3, 3, 3, 3, 2, 2: one code 16 writes the 3 of 258 and of distance symbols 0 .. 3
    r16_ll, r16_dd = _lens(259, {97: 1, 256: 2, 257: 3, 258: 3}), [3, 3, 3, 3, 2, 2]
    r16_cl = dw.with_run(r16_ll + r16_dd, 258, 16, 5)
    # 259 .. 261 and distance symbols 0, 1 have no code: one code 17 writes those five zeros
    r17_ll, r17_dd = _lens(262, {97: 1, 256: 2, 257: 3, 258: 3}), [0, 0, 1, 1]
    r17_cl = dw.with_run(r17_ll + r17_dd, 259, 17, 5)
    plain_ll, plain_dd = _lens(258, {97: 1, 256: 2, 257: 2}), [1, 1]
    ten = _rbytes(r, 10)
    good = [
        ("all_symbols", _all_symbols(dw)),
        ("one_dist_code", [dw.dynamic([A, Bb, (M, 257, 0, 0, 0), Bb, (M, 285, 0, 0, 0), A, (M, 284, 31, 0, 0), (M, 264, 0, 0, 0), EOB], one_ll, [1])]),
        ("empty_dist", [dw.dynamic(list(b"no distance code at all") + [EOB], lit_ll, [0])]),
        ("only_eob", [dw.dynamic([EOB], _lens(257, {256: 1}), [0])]),
        ("rep16_crosses", [dw.dynamic([97, 97, 97, dw.match(4, 1), dw.match(3, 6), 97, dw.match(4, 5), dw.match(3, 7), EOB], r16_ll, r16_dd, r16_cl)]),
        ("rep17_crosses", [dw.dynamic([97, 97, 97, dw.match(3, 3), 97, dw.match(4, 4), EOB], r17_ll, r17_dd, r17_cl)]),
        ("dist_10_of_10", [dw.stored(ten), dw.fixed([dw.match(20, 10), EOB])]),
        ("many_blocks", _many_blocks(dw)),
    ]
    for k in range(8):  # 3 + 9 k + 7 bits of fixed block in front of the stored header: bit (2 + k) mod 8
        for n in STORED_ALIGN_N:
            good.append(("stored_align%d_%d" % (k, n), [dw.fixed([144 + r.randrange(112) for _ in range(k)] + [EOB]), dw.stored(_rbytes(r, n))]))
    for n in STORED_IN_N:
        good.append(("stored_in%d" % n, [dw.stored(_rbytes(r, n - 5))]))
    pad = (B, 0, 16)
    bad = [
        ("one_dist_code_unused_bit", [dw.dynamic([A, Bb, (S, "ll", 257), (B, 1, 1), A, EOB, pad], one_ll, [1])]),
        ("empty_dist_used", [dw.dynamic([A, Bb, (S, "ll", 257), pad, EOB], lit257_ll, [0])]),
        ("only_eob_unused_bit", [dw.dynamic([(B, 1, 1), pad], _lens(257, {256: 1}), [0])]),
        ("first_is_16", [dw.dynamic([97, EOB], plain_ll, plain_dd, [(16, 3)] + (plain_ll + plain_dd)[3:])]),
        ("repeat_overruns", [dw.dynamic([97, EOB], plain_ll, plain_dd, (plain_ll + plain_dd)[:-2] + [(18, 11)])]),
        ("no_eob", [dw.dynamic([97, 98, pad], _lens(257, {97: 1, 98: 1}), [1, 1])]),
        ("incomplete_ll", [dw.dynamic([97, EOB, pad], _lens(257, {97: 2, 256: 2}), [1, 1])]),
        ("oversub_ll", [dw.dynamic([97, EOB, pad], _lens(257, {97: 1, 98: 1, 256: 1}), [1, 1])]),
        ("fixed_286", [dw.fixed([A, (S, "ll", 286), pad, EOB])]),
        ("fixed_dist30", [dw.fixed([A, Bb, A, (S, "ll", 257), (S, "dd", 30), pad, EOB])]),
        ("dist_11_of_10", [dw.stored(ten), dw.fixed([dw.match(20, 11), EOB])]),
        ("hdist_31", [dw.dynamic([97, EOB, pad], plain_ll, dw.random_complete(r, range(31), 15, 31))]),
    ]
    return good, bad


def _first_coded_byte(dw, blocks):
    """the byte in which the first block that is not stored begins (0 if all are)"""
    starts = []
    dw.write(blocks, starts)
    return next((s >> 3 for s, b in zip(starts, blocks) if b[0] != "stored"), 0)


@functools.lru_cache(maxsize=None)
def crafted_set():
    """(good, bad) lists of (name, data, size) made with tests/deflate_writer.py: streams that are valid (or precisely not) by RFC 1951
    but that zlib's deflate does not write.  `size` is what the writer's tokens come to; what a decoder must do with a member is the
    yardstick's -- zlib's -- word, see check_crafted_set.
      good  all_symbols (see _all_symbols), one_dist_code, empty_dist, only_eob (a literal/length set of the end-of-block code alone: no
            output), rep16_crosses / rep17_crosses (one repeat code writes the last literal/length and the first distance lengths),
            dist_10_of_10, many_blocks, stored_align{k}_{n} (a stored header at every bit position, n stored bytes), stored_in{n} (a
            stored member of n input bytes, around the 1 KiB input chunks)
      bad   the other code of a single-code set used (one_dist_code_unused_bit, only_eob_unused_bit), a match with no distance code
            (empty_dist_used), code 16 first, a repeat running over HLIT + HDIST, no end-of-block code, an incomplete and an
            over-subscribed literal/length set, symbol 286 and distance symbol 30 in a fixed block, a distance one beyond the bytes so
            far, HDIST 31"""
    from tests import deflate_writer as dw
    good, bad = _crafted()
    return tuple([(name, dw.write(blocks), len(dw.apply(blocks, part is good))) for name, blocks in part] for part in (good, bad))


def check_crafted_set():
    """zlib's verdict on every crafted member, and -- by the profiler's own decoder -- the decoder paths the good ones are there for.  A
    member that is simplified until a path is lost fails here."""
    from tests import deflate_writer as dw
    good, bad = crafted_set()
    assert len({n for n, _, _ in good + bad}) == len(good) + len(bad) == 8 + 8 * len(STORED_ALIGN_N) + len(STORED_IN_N) + 12
    for n, m, s in good:
        assert yardstick(m, s)[0], n
    for n, m, s in bad:
        assert not yardstick(m, s)[0], n
    prof = {n: dw.profile(m) for n, m, s in good}
    for n, m, s in good:
        assert prof[n]["out"] == yardstick(m, s)[1], n  # the profiler reads the stream as zlib does
    for n, m, s in bad:
        try:
            dw.profile(m)
        except ValueError:
            continue
        raise AssertionError("the profiler accepts " + n)
    every = list(prof.values())
    assert set().union(*(p["len_symbols"] for p in every)) == set(range(257, 286))
    assert set().union(*(p["dist_symbols"] for p in every)) == set(range(30))
    assert max(p["ll_bits_in_match"] for p in every) == 15 and max(p["dd_bits_in_match"] for p in every) == 15
    assert sum(p["repeats_crossing"] for p in every) >= 1
    assert sum(p["single_dist_sets"] for p in every) >= 1 and sum(p["empty_dist_sets"] for p in every) >= 1
    assert sum(p["single_ll_sets"] for p in every) >= 1
    assert {b % 8 for p in every for b in p["stored_bits"]} == set(range(8))
    for d in (63, 64, 65):
        assert max(p["len_at_dist"][d] for p in every) >= 258, d
    # member by member: what each one is there for
    a = prof["all_symbols"]
    assert a["blocks"] == ["stored", "dynamic"] and a["len_symbols"] == set(range(257, 286)) and a["dist_symbols"] == set(range(30))
    assert (a["ll_bits_in_match"], a["dd_bits_in_match"]) == (15, 15) and a["len_at_dist"] == {63: 258, 64: 258, 65: 258}
    assert 32768 + 256 < len(a["out"]) <= MAX_OUT and set(a["out"][32768:32768 + 256]) == set(range(256))
    assert prof["one_dist_code"]["single_dist_sets"] == 1 and 285 in prof["one_dist_code"]["len_symbols"]
    assert prof["empty_dist"]["empty_dist_sets"] == 1 and not prof["empty_dist"]["len_symbols"]
    assert prof["only_eob"]["single_ll_sets"] == 1 and prof["only_eob"]["out"] == b""
    assert prof["rep16_crosses"]["repeats_crossing"] == 1 and prof["rep17_crosses"]["repeats_crossing"] == 1
    assert prof["dist_10_of_10"]["blocks"] == ["stored", "fixed"] and len(prof["dist_10_of_10"]["out"]) == 30
    m = prof["many_blocks"]
    assert m["blocks"] == ["dynamic"] * 200 and len(m["out"]) <= MAX_OUT
    assert len({b // 8192 for b in m["block_bits"]}) >= 20  # block headers in (and across) many 1 KiB input chunks
    d = {n: (m_, s) for n, m_, s in good}
    for k in range(8):
        for n in STORED_ALIGN_N:
            p = prof["stored_align%d_%d" % (k, n)]
            assert p["blocks"] == ["fixed", "stored"] and p["stored_bits"][0] % 8 == (2 + k) % 8 and len(p["out"]) == k + n
    for n in STORED_IN_N:
        assert len(d["stored_in%d" % n][0]) == n and prof["stored_in%d" % n]["blocks"] == ["stored"]


CRAFTED_SWEEP_SEED = 1951


@functools.lru_cache(maxsize=None)
def crafted_sweep():
    """the mutation sweep of the crafted members (all but stored_align* and stored_in*): of each, 150 single-bit flips -- seven in ten
    of them in the first 96 bytes of its first block that is not stored, where the header checks are -- and 20 truncations.  List of
    (data, size), shuffled; the GPU tests run the first 300.  By zlib (crafted_sweep_verdicts), with seed CRAFTED_SWEEP_SEED:
    244 of the 3 400 cases are accepted and 3 156 rejected; of the first 300, 21 and 279."""
    from tests import deflate_writer as dw
    good, bad = _crafted()
    r = random.Random(CRAFTED_SWEEP_SEED)
    cases = []
    for name, blocks in good + bad:
        if name.startswith("stored_"):
            continue
        data, size, head = dw.write(blocks), len(dw.apply(blocks, False)), _first_coded_byte(dw, blocks)
        for _ in range(150):
            at = head * 8 + r.randrange(8 * min(96, len(data) - head)) if r.random() < 0.7 else r.randrange(8 * len(data))
            m = bytearray(data)
            m[at >> 3] ^= 1 << (at & 7)
            cases.append((bytes(m), size))
        for _ in range(20):
            cases.append((data[:r.randrange(len(data))], size))
    r.shuffle(cases)
    return cases


@functools.lru_cache(maxsize=None)
def crafted_sweep_verdicts():
    return [yardstick(m, s) for m, s in crafted_sweep()]


def check_crafted_sweep():
    """a condition, not a measurement: enough cases of either verdict in the whole sweep and in the GPU's share of it"""
    v = [ok for ok, _ in crafted_sweep_verdicts()]
    assert len(v) == 3400
    assert min(sum(v), len(v) - sum(v)) >= 100, (sum(v), len(v))
    assert min(sum(v[:300]), 300 - sum(v[:300])) >= 10, sum(v[:300])


FOREIGN_NAMES = ("reads150b_level1", "reads150b_level12", "reads5kb_level1", "reads5kb_level12")


def foreign_texts():
    from tests import deflate_cases as dc
    return {"reads150b": dc.fastq_150b(20000), "reads5kb": dc.fastq_5kb(20000)}


@functools.lru_cache(maxsize=None)
def foreign_set():
    """list of (name, data, size, crc): raw deflate members written by libdeflate, not zlib -- tests/golden/foreign_members.bin, made by
    tests/golden/make_foreign_members.py.  The file is a count, then for each member its input length, output length and CRC-32
    (little-endian 32-bit words) and its bytes."""
    import os
    import struct
    blob = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foreign_members.bin"), "rb").read()
    (n,), at, out = struct.unpack_from("<I", blob, 0), 4, []
    assert n == len(FOREIGN_NAMES)
    for name in FOREIGN_NAMES:
        in_len, out_len, crc = struct.unpack_from("<III", blob, at)
        out.append((name, blob[at + 12:at + 12 + in_len], out_len, crc))
        at += 12 + in_len
    assert at == len(blob)
    return out


def check_foreign_set():
    """zlib inflates every foreign member to the seeded text, and the CRC-32 of the fixture is that text's; they hold what zlib's
    members lack: length symbols with 2 and more extra bits out of dynamic tables, dynamic blocks with nothing between them"""
    from tests import deflate_writer as dw
    texts = foreign_texts()
    for name, m, s, crc in foreign_set():
        want = texts[name.split("_")[0]]
        assert s == len(want) == 20000 and yardstick(m, s) == (True, want), name
        assert crc == (zlib.crc32(want) & 0xFFFFFFFF), name
        p = dw.profile(m)
        assert p["out"] == want and set(p["blocks"]) == {"dynamic"}, name
        if name.startswith("reads150b"):  # (the 5 kb reads are random letters: few matches, and short ones)
            assert len(p["len_symbols"]) >= 24 and max(p["len_symbols"]) >= 281, (name, sorted(p["len_symbols"]))
        if name == "reads5kb_level12":
            assert p["blocks"] == ["dynamic"] * 3


def bgzf(data, level=6, block=65280):
    """`data` as a BGZF file (SAM specification 4.1): members of `block` bytes and the empty end-of-file member"""
    import struct
    out = b""
    for at in list(range(0, len(data), block)) + [len(data)]:
        c = data[at:at + block]
        z = raw(c, level)
        out += (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(z) + 8 - 1) + z +
                struct.pack("<II", zlib.crc32(c) & 0xFFFFFFFF, len(c)))
    return out
