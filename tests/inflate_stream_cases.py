"""The cases of the stream-inflate tests (tests/test_inflate_stream_cpu.py, tests/test_gpu_inflate_stream.py): raw deflate streams with
known block starts, cut into chunks, and what chn_inflate_stream_run[_host] must report for them.  The bytes are always zlib's
(zlib.decompressobj(-15) over the whole stream, with the window as its dictionary where a case starts later), the CRCs zlib.crc32's;
where a chunk's bytes end follows from how the stream was made -- the Z_SYNC_FLUSH points of zlib.compressobj (byte-aligned block
starts that matches cross), or the blocks handed to tests/deflate_writer.py (any bit alignment, streams zlib never writes).
Everything is seeded.  A case is a dict:
    data, begin, target, window, kw   the job (kw: sym_capacity, out_bytes)
    n_counted, lengths, status, final what the counted chunks must report; end_bit: per chunk a bit position or None (not pinned)
    text                              out[:out_used]"""
import functools
import random
import zlib

from tests import deflate_writer as dw
from tests import inflate_cases as ic

MIN_SYMS = 131072
E_ROOM = 8
EOB = dw.EOB


def crc_join(a, b, n):
    """crc32(A + B) from crc32(A), crc32(B) and len(B), by zlib.crc32 alone (the CRC is linear: A|B = A|0..0 xor 0..0|B)"""
    z = bytes(n)
    return zlib.crc32(z, a) ^ zlib.crc32(z) ^ b


def make(name, data, begin, target, lengths, text, status=None, final=None, end_bit=None, window=b"", n_counted=None, **kw):
    n = len(lengths)
    c = dict(name=name, data=bytes(data), begin=list(begin), target=list(target), window=bytes(window), lengths=list(lengths),
             status=list(status) if status is not None else [0] * n, final=list(final) if final is not None else [0] * n,
             end_bit=list(end_bit) if end_bit is not None else [None] * n, n_counted=n if n_counted is None else n_counted, kw=dict(kw))
    total = sum(lengths)
    assert len(text) >= total
    c["text"] = bytes(text[:total])
    c["kw"].setdefault("out_bytes", total + 77)
    c["kw"].setdefault("sym_capacity", max(MIN_SYMS, len(text)))  # (no chunk of the case is short of symbols, unless the case says so)
    assert len(c["begin"]) == len(c["target"]) >= n
    return c


def check(res, c):
    """res: the dict of api.inflate_stream_host / Inflater.run_stream"""
    name = c["name"]
    assert res["n_counted"] == c["n_counted"], (name, res["n_counted"], res["status"], res["end_bit"], c["begin"])
    assert res["status"] == c["status"], (name, res["status"])
    assert res["out_length"] == c["lengths"], (name, res["out_length"])
    assert res["final"] == c["final"], (name, res["final"])
    assert res["out_used"] == sum(c["lengths"]), name
    for got, want in zip(res["end_bit"], c["end_bit"]):
        assert want is None or got == want, (name, res["end_bit"], c["end_bit"])
    if res["bytes"] is not None:
        assert res["bytes"] == c["text"], name
    at, joined = 0, 0
    for n, crc in zip(c["lengths"], res["crc32"]):
        assert crc == zlib.crc32(c["text"][at:at + n]), (name, at)
        joined = crc_join(joined, crc, n)
        at += n
    assert joined == zlib.crc32(c["text"]), name


def same(dev, host, name=""):
    """the device's results against the host form's, field by field (the counted chunks)"""
    for k in ("n_counted", "out_used", "end_bit", "out_length", "status", "final", "crc32"):
        assert dev[k] == host[k], (name, k, dev[k], host[k])
    if dev["bytes"] is not None:
        assert dev["bytes"] == host["bytes"], name


# ---- streams zlib writes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fastq():
    return ic.fastq_text(600000, 11)


@functools.lru_cache(maxsize=None)
def zstream(which, level, strategy, every, first=None):
    """(data, cuts): `which` text deflated raw with a sync flush every `every` bytes (the first after `first`); cuts = [(text offset,
    data offset)] of the stream's start and of every flush point -- each a byte-aligned block start"""
    text = {"fastq": fastq, "lines": repeating_lines, "small": lambda: ic.fastq_text(61000, 5)}[which]()
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, cuts, at = b"", [(0, 0)], 0
    while at < len(text):
        step = first if (at == 0 and first) else every
        out += c.compress(text[at:at + step])
        at += step
        if at < len(text):
            out += c.flush(zlib.Z_SYNC_FLUSH)
            cuts.append((at, len(out)))
    return out + c.flush(), cuts, text


@functools.lru_cache(maxsize=None)
def repeating_lines():
    """every line repeats the line 200 bytes before it, but for one character: markers live on to a chunk's last bytes"""
    r = random.Random(31)
    line = bytearray(r.choice(b"ACGTFF:,#") for _ in range(199)) + b"\n"
    out = bytearray()
    for i in range(1500):
        line[r.randrange(199)] = r.choice(b"ACGT")
        out += line
    return bytes(out)


def zcase(name, which, level, strategy, every, pick, start=0, window=None, first=None, **kw):
    """chunks at the flush points pick(cuts) of a zlib stream, from flush point `start` on; window: how many bytes of the true text in
    front of it the job gets (None: all 32 768 that exist).  With a short window the verdict is zlib's, chunk by chunk: each chunk's
    data inflated with the bytes a decoder has by then as the dictionary -- an error there is status 4 with no progress."""
    data, cuts, text = zstream(which, level, strategy, every, first)
    cuts = [c for i, c in enumerate(cuts) if i >= start]
    cuts = [cuts[0]] + [c for c in pick(cuts[1:])]
    t0, d0 = cuts[0]
    have = min(t0, 32768) if window is None else window
    assert have <= t0
    win = text[t0 - have:t0]
    begin = [8 * (d - d0) for _, d in cuts]
    target = begin[1:] + [8 * (len(data) - d0)]
    ends = [t for t, _ in cuts[1:]] + [len(text)]
    lengths, status, final, end_bit = [], [], [], []
    hist = win
    for k, ((t, d), te) in enumerate(zip(cuts, ends)):
        dend = cuts[k + 1][1] if k + 1 < len(cuts) else len(data)
        o = zlib.decompressobj(-15, zdict=hist[-32768:]) if hist else zlib.decompressobj(-15)
        try:
            got = o.decompress(data[d:dend])
        except zlib.error as e:
            assert "too far back" in str(e) and window is not None
            lengths.append(0); status.append(4); final.append(0); end_bit.append(begin[k])
            break
        assert got == text[t:te]
        lengths.append(te - t); status.append(0); final.append(1 if k + 1 == len(cuts) else 0)
        end_bit.append(target[k] if k + 1 < len(cuts) else None)
        hist = (hist + got)[-32768:]
    c = make(name, data[d0:], begin, target, lengths, text[t0:], status, final, end_bit, window=win, **kw)
    if status[-1] == 0:
        assert 8 * (len(data) - d0) - 8 < 1 << 62  # (the last chunk ends inside the stream's last byte; checked by the tests)
        c["last_byte"] = len(data) - d0
    return c


EVERY = lambda cuts: cuts
THIRD = lambda cuts: cuts[2::3]
NONE = lambda cuts: []
FLAVOURS = [("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
            ("fixed", 6, zlib.Z_FIXED), ("rle", 6, zlib.Z_RLE)]


def fastq_cases():
    out = []
    for fname, level, strategy in FLAVOURS:
        for pname, pick in (("every", EVERY), ("third", THIRD), ("one", NONE)):
            out.append(zcase("fastq_%s_%s" % (fname, pname), "fastq", level, strategy, 40000, pick))
            out.append(zcase("fastq_%s_%s_from5" % (fname, pname), "fastq", level, strategy, 40000, pick, start=5))
            out.append(zcase("fastq_%s_%s_from5_w1000" % (fname, pname), "fastq", level, strategy, 40000, pick, start=5, window=1000))
    return out


def stored_cases():
    """level 0: stored blocks -- two of 65 535 bytes in front of the first flush -- and the empty block of a sync flush alone in a chunk"""
    data, cuts, text = zstream("fastq", 0, zlib.Z_DEFAULT_STRATEGY, 40000, 150000)
    assert data[0] == 0 and data[1:5] == b"\xff\xff\x00\x00"  # a stored block of 65 535 bytes comes first
    out = [zcase("stored_every", "fastq", 0, zlib.Z_DEFAULT_STRATEGY, 40000, EVERY, first=150000)]
    (t1, d1), (t2, d2) = cuts[1], cuts[2]
    assert data[d1 - 5:d1] == b"\x00\x00\x00\xff\xff"
    begin = [0, 8 * (d1 - 5), 8 * d1, 8 * d2]
    target = begin[1:] + [8 * len(data)]
    lengths = [t1, 0, t2 - t1, len(text) - t2]
    out.append(make("stored_empty_block_alone", data, begin, target, lengths, text, final=[0, 0, 0, 1], end_bit=target[:3] + [None]))
    return out


def lines_cases():
    return [zcase("lines_every", "lines", 6, zlib.Z_DEFAULT_STRATEGY, 40000, EVERY), zcase("lines_l1_third", "lines", 1, zlib.Z_DEFAULT_STRATEGY, 20000, THIRD)]


def many_chunks(n):
    """n chunks of about 100 bytes of text each (n <= 610): flush points 100 bytes apart"""
    def pick(cuts):
        return cuts[:n - 1]
    return zcase("many_%d" % n, "small", 6, zlib.Z_DEFAULT_STRATEGY, 100, pick)


# ---- streams made with the writer ----------------------------------------------------------------------------------------------------
def _rbytes(r, n, alphabet=None):
    return bytes(r.choice(alphabet) for _ in range(n)) if alphabet else bytes(r.randrange(256) for _ in range(n))


def wcase(name, blocks, firsts, n_counted=None, **kw):
    """a writer stream cut into chunks that begin with blocks `firsts` (indices, the first is 0): all proven, the last one final"""
    starts = []
    data = dw.write(blocks, starts)
    text = zlib.decompressobj(-15).decompress(data)
    sizes = [len(dw.apply(blocks[:i])) for i in firsts] + [len(dw.apply(blocks))]
    assert sizes[-1] == len(text)
    begin = [starts[i] for i in firsts]
    target = begin[1:] + [8 * len(data)]
    n = len(firsts)
    return make(name, data, begin, target, [sizes[k + 1] - sizes[k] for k in range(n)], text, final=[0] * (n - 1) + [1],
                end_bit=target[:n - 1] + [None], **kw)


def distance_cases():
    r = random.Random(41)
    head = dw.stored(_rbytes(r, 40000))
    out = []
    toks = []
    for dist in (32768, 32767, 32705, 32704):
        for length in (3, 258):
            toks += list(_rbytes(r, 3)) + [dw.match(length, dist)]
    out.append(wcase("far_matches_at_chunk_start", [head, dw.fixed(toks + [EOB])], [0, 1]))
    out.append(wcase("far_match_first", [head, dw.fixed([dw.match(258, 32768), dw.match(3, 32768), EOB])], [0, 1]))
    # a source that straddles the chunk start: ten literals, then matches that begin 15 bytes in front of the chunk
    out.append(wcase("straddle", [head, dw.fixed(list(_rbytes(r, 10)) + [dw.match(20, 25), 7, dw.match(258, 36), 9, dw.match(258, 300), EOB])], [0, 1]))
    # overlapping matches whose source begins in the window
    toks = []
    for dist in (1, 2, 63, 64, 65):
        toks += [dw.match(258, dist), dw.match(3, dist + 258 + 3), 65 + dist % 26]
    out.append(wcase("overlap_from_window", [head, dw.fixed([dw.match(258, 1)] + toks + [EOB])], [0, 1]))
    for dist in (1, 2, 63, 64, 65):
        out.append(wcase("overlap_%d_first" % dist, [head, dw.fixed([dw.match(258, dist), dw.match(100, dist), EOB])], [0, 1]))
    # ring wrap: more than 32 768 symbols in the chunk, then matches over the distances at which source and destination share a slot
    toks = list(_rbytes(r, 33000, b"ACGTN\n"))
    for rep in range(3):
        for dist in (32768, 32767, 32705, 32704, 32736):
            for length in (3, 258, 64, 65):
                toks += [dw.match(length, dist)] + list(_rbytes(r, 1 + (rep + length) % 5, b"acgt"))
        toks += [dw.match(258, 32768)] * 120  # another 30 960 symbols: the ring wraps again before the next round
    out.append(wcase("ring_wrap", [head, dw.fixed(toks + [EOB])], [0, 1]))
    out.append(wcase("ring_wrap_one_chunk", [head, dw.fixed(toks + [EOB])], [0]))
    return out


def alignment_cases():
    """one chunk a block, blocks of odd sizes in bits: block starts at all eight bit alignments (asserted), each chunk with a match
    into the chunk in front of it"""
    r = random.Random(43)
    blocks = [dw.fixed(list(_rbytes(r, 300, b"ACGT")) + [EOB])]
    for k in range(24):
        blocks.append(dw.fixed(list(_rbytes(r, 5 + k, b"ACGT")) + [200] * (k % 3) + [dw.match(30 + k, 40 + 3 * k), EOB]))
    starts = []
    dw.write(blocks, starts)
    assert {s % 8 for s in starts} == set(range(8))
    out = [wcase("all_alignments", blocks, list(range(len(blocks))))]
    dyn = []
    for k in range(9):  # the same with dynamic blocks (their headers are 17 bits and more of fields that are not byte-sized)
        lits = sorted(set(b"ACGTN\n"))
        ll = dw.random_complete(r, lits + [256, 257 + k, 285], 9, 286)
        dd = dw.random_complete(r, sorted({3 + k, 10, 29}), 4, 30)
        toks = [lits[r.randrange(len(lits))] for _ in range(40 + k)] + [dw.match(3 + k if k < 8 else 11, dw.DIST_BASE[3 + k]), EOB]
        dyn.append(dw.dynamic(toks, ll, dd))
    out.append(wcase("dynamic_alignments", [blocks[0]] + dyn, list(range(10))))
    return out


def one_symbol_blocks():
    r = random.Random(47)
    blocks = [dw.fixed([r.choice(b"ACGT"), EOB]) for _ in range(200)] + [dw.fixed([dw.match(100, 60), EOB])]
    return [wcase("one_symbol_blocks", blocks, [0, 1, 2, 3, 50, 100, 150, 200]), wcase("one_symbol_blocks_each", blocks[:70] + blocks[-1:], list(range(71)))]


def _six_blocks():
    r = random.Random(53)
    blocks = [dw.fixed(list(_rbytes(r, 200 + 10 * k, b"ACGT\n")) + ([dw.match(50, 120)] if k else []) + [EOB]) for k in range(6)]
    starts = []
    data = dw.write(blocks, starts)
    sizes = [len(dw.apply(blocks[:i])) for i in range(7)]
    return blocks, data, starts, sizes, zlib.decompressobj(-15).decompress(data)


def chain_cases():
    blocks, data, starts, sizes, text = _six_blocks()
    out = []
    # chunk 2 begins four bits inside block 3: chunk 1 decodes on to the end of that block and does not stand on it; two chunks count
    begin = [starts[0], starts[2], starts[3] + 4, starts[5]]
    out.append(make("begin_inside_a_block", data, begin, begin[1:] + [8 * len(data)], [sizes[2], sizes[4] - sizes[2]], text,
                    end_bit=[starts[2], starts[4]]))
    # a target inside block 1: the chunk stands at that block's end, where the next chunk begins
    begin = [starts[0], starts[2], starts[4]]
    out.append(make("target_inside_a_block", data, begin, [starts[1] + 9, starts[3] + 1, 8 * len(data)],
                    [sizes[2], sizes[4] - sizes[2], sizes[6] - sizes[4]], text, final=[0, 0, 1], end_bit=[starts[2], starts[4], None]))
    # a final block in a middle chunk, bytes behind it, and a chunk that begins among those
    more = data + bytes(random.Random(59).randrange(256) for _ in range(64))
    begin = [starts[0], starts[4], 8 * len(data) + 16, 8 * len(data) + 77]
    out.append(make("final_in_the_middle", more, begin, begin[1:] + [8 * len(more)], [sizes[4], sizes[6] - sizes[4]], text, final=[0, 1],
                    end_bit=[starts[4], None]))
    return out


def _bits(data, n):
    return [(data[i >> 3] >> (i & 7)) & 1 for i in range(n)]


def _pack(bits):
    w = ic.BitWriter()
    w.bits = list(bits)
    return w.bytes()


def _field(value, n):
    return [(value >> i) & 1 for i in range(n)]


def corrupt_kinds():
    """name -> (what stands where the third block of the chunk should: a writer block, or raw bits; the status)"""
    S = dw.SYM
    lens = ic._lens
    return {
        "type3": ([0, 1, 1], 2),
        "stored_nlen": ("stored_nlen", 2),
        "oversubscribed": (dw.dynamic([65, EOB], lens(257, {65: 1, 66: 1, 256: 1}), [1, 1]), 3),
        "incomplete": (dw.dynamic([65, EOB], lens(257, {65: 2, 256: 2}), [1, 1]), 3),
        "no_eob": (dw.dynamic([65, 66], lens(257, {65: 1, 66: 1}), [1, 1]), 3),
        "dist30": (dw.fixed([65, 66, 67, (S, "ll", 257), (S, "dd", 30), EOB]), 4),
        "cut": ("cut", 1),
    }


def corrupt_case(kind, at):
    """four chunks of two good blocks each; the third block of chunk `at` is corrupt (the chunks behind it begin inside it: unproven)"""
    bad, status = corrupt_kinds()[kind]
    r = random.Random(61)
    good = [dw.fixed(list(_rbytes(r, 150 + 7 * k, b"ACGT\n")) + ([dw.match(40, 100)] if k else []) + [EOB]) for k in range(2 * at + 2)]
    tail = dw.fixed(list(_rbytes(r, 300, b"ACGT")) + [EOB])
    starts = []
    data = dw.write(good + [bad if isinstance(bad, tuple) else tail, dw.fixed([EOB])], starts)
    s_bad = starts[len(good)]
    if kind == "cut":
        data = data[:(s_bad >> 3) + 20]  # inside the third block
    elif not isinstance(bad, tuple):
        bits = _bits(data, s_bad)
        if bad == "stored_nlen":
            bits += [0, 0, 0]
            bits += [0] * (-len(bits) % 8) + _field(5, 16) + _field(5, 16)
        else:
            bits += bad
        data = _pack(bits + [0] * 400)
    text = zlib.decompressobj(-15).decompress(dw.write(good + [dw.fixed([EOB])]))
    sizes = [len(dw.apply(good[:i])) for i in range(len(good) + 1)]
    begin = [starts[2 * k] for k in range(at + 1)]
    begin += [s_bad + 9 * (i + 1) for i in range(3 - at)]
    assert begin[-1] < 8 * len(data)
    target = begin[1:] + [8 * len(data)]
    lengths = [sizes[2 * k + 2] - sizes[2 * k] for k in range(at + 1)]
    return make("corrupt_%s_in_chunk_%d" % (kind, at), data, begin, target, lengths, text, status=[0] * at + [status],
                end_bit=[starts[2 * k + 2] for k in range(at + 1)])


def corrupt_cases():
    return [corrupt_case(kind, at) for kind in corrupt_kinds() for at in (0, 2)]


def too_far_cases():
    r = random.Random(67)
    out = []
    blocks = [dw.fixed(list(_rbytes(r, 5, b"ACGT")) + [dw.match(3, 10), EOB])]
    data = dw.write(blocks)
    out.append(make("too_far_in_chunk_0", data, [0], [8 * len(data)], [0], b"", status=[4], end_bit=[0]))
    # ... and with 5 bytes of window: it reaches exactly the first of them
    blocks = [dw.fixed(list(_rbytes(r, 5, b"ACGT")) + [dw.match(3, 10), EOB])]
    data = dw.write(blocks)
    text = zlib.decompressobj(-15, zdict=b"WINDO").decompress(data)
    out.append(make("just_in_reach_in_chunk_0", data, [0], [8 * len(data)], [8], text, final=[1], window=b"WINDO"))
    # through a marker: 100 bytes of member in front of chunk 1, whose match reaches 195 in front of it
    lits = list(_rbytes(r, 100, b"ACGT"))
    starts = []
    data = dw.write([dw.fixed(lits + [EOB]), dw.fixed(list(_rbytes(r, 5, b"ACGT")) + [dw.match(3, 200), EOB])], starts)
    out.append(make("too_far_through_a_marker", data, starts, [starts[1], 8 * len(data)], [100, 0], bytes(lits), status=[0, 4],
                    end_bit=[starts[1], starts[1]]))
    # the same reaching the member's very first byte: fine
    starts = []
    blocks = [dw.fixed(lits + [EOB]), dw.fixed(list(_rbytes(r, 5, b"ACGT")) + [dw.match(3, 105), EOB])]
    data = dw.write(blocks, starts)
    out.append(make("just_in_reach_through_a_marker", data, starts, [starts[1], 8 * len(data)], [100, 8], zlib.decompressobj(-15).decompress(data),
                    final=[0, 1], end_bit=[starts[1], None]))
    return out


@functools.lru_cache(maxsize=None)
def _big_block():
    """one block of more than a million symbols: a zero, then 4 100 matches of length 258 at distance 1"""
    return dw.fixed([0] + [dw.match(258, 1)] * 4100 + [EOB])


def capacity_cases():
    r = random.Random(71)
    a, b = dw.fixed(list(_rbytes(r, 500, b"ACGT")) + [EOB]), dw.fixed(list(_rbytes(r, 700, b"ACGT")) + [dw.match(100, 1000), EOB])
    out = []
    data = dw.write([_big_block(), dw.fixed([EOB])])
    out.append(make("capacity_block_first", data, [0], [8 * len(data)], [0], b"", status=[5], end_bit=[0], sym_capacity=MIN_SYMS))
    starts = []
    data = dw.write([a, b, _big_block(), dw.fixed([EOB])], starts)
    text = bytes(dw.apply([a, b]))
    assert zlib.decompressobj(-15).decompress(data)[:1300] == text and len(text) == 1300
    out.append(make("capacity_block_third", data, [0], [8 * len(data)], [1300], text, status=[5], end_bit=[starts[2]], sym_capacity=MIN_SYMS))
    # ... and with room for it all, the same stream decodes: the capacity was the reason
    whole = zlib.decompressobj(-15).decompress(data)
    out.append(make("capacity_enough", data, [0], [8 * len(data)], [len(whole)], whole, final=[1], sym_capacity=len(whole)))
    return out


def room_case():
    """out_bytes one byte short of chunk 1"""
    c = zcase("no_room_for_chunk_1", "fastq", 6, zlib.Z_DEFAULT_STRATEGY, 40000, lambda cuts: cuts[:3])
    c["kw"]["out_bytes"] = c["lengths"][0] + c["lengths"][1] - 1
    c["lengths"], c["status"], c["final"] = [c["lengths"][0], 0], [0, E_ROOM], [0, 0]
    c["end_bit"] = [c["begin"][1], c["begin"][1]]
    c["n_counted"] = 2
    c["text"] = c["text"][:c["lengths"][0]]
    c.pop("last_byte", None)
    return c


def crafted_cases():
    return (distance_cases() + alignment_cases() + one_symbol_blocks() + chain_cases() + corrupt_cases() + too_far_cases() + capacity_cases()
            + [room_case()])


def run(fn, c, **more):
    """fn: api.inflate_stream_host or an Inflater's run_stream"""
    kw = dict(c["kw"])
    kw.update(more)
    res = fn(c["data"], c["begin"], c["target"], window=c["window"], **kw)
    if "last_byte" in c and res["n_counted"] == len(c["begin"]):  # the final block ends inside the stream's last byte
        assert 8 * c["last_byte"] - 8 < res["end_bit"][-1] <= 8 * c["last_byte"], c["name"]
    return res
