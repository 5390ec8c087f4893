"""The member set of the inflate tests (tests/test_inflate_cpu.py, tests/test_gpu_inflate.py): small raw deflate members made with
Python's zlib or a bit writer, and the yardstick that says which of them a decoder must accept -- Python's zlib, never the code under
test.  Everything is seeded, so both test files see the same bytes."""
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
