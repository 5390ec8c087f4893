"""The pieces of the deflate tests (tests/test_deflate_cpu.py, tests/test_gpu_deflate.py): the smallest shapes at which a member
compressor can go wrong, and three FASTQ fixtures cut into pieces of 65 280 bytes.  The yardstick is Python's zlib and gzip, never the
code under test.  Everything is seeded, so both test files see the same bytes."""
import functools
import gzip
import os
import random
import struct
import zlib

import numpy as np

MAX_IN = 65280
HERE = os.path.dirname(os.path.abspath(__file__))


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _far_repeat(distance):
    """`distance` random bytes, then their beginning again up to 65 280 bytes: the only repeat lies `distance` back"""
    head = _rand(distance, 1000 + distance)
    return head + head[:MAX_IN - distance]


@functools.lru_cache(maxsize=None)
def shapes():
    """[(name, bytes)]"""
    text = fastq_5kb(MAX_IN)
    out = [("len%d" % n, text[:n]) for n in (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 258, 259, 260, 32767, 32768, 32769, 65279, 65280)]
    out += [("run%d" % n, b"Q" * n) for n in (2, 259, 1000, MAX_IN)]                  # distance 1, overlapping copies, chains of 258
    for period in (2, 3, 63, 64, 65):
        unit = _rand(period, period)
        out.append(("period%d" % period, (unit * (3000 // period + 1))[:3000]))
    rec = fastq_5kb(300)
    out.append(("record300", (rec * (MAX_IN // 300 + 1))[:MAX_IN]))
    out.append(("far40000", _far_repeat(40000)))                                       # beyond 32 768: zlib rejects a far distance
    out.append(("far32768", _far_repeat(32768)))
    out.append(("far32769", _far_repeat(32769)))
    for d in (32768, 32769):                                                           # a key, a run that leaves its table entry alone, the key again
        out.append(("edge%d" % d, _rand(16, 3) + b"\0" * (d - 16) + _rand(16, 3) + b"\0" * 100))
    out.append(("noise", _rand(MAX_IN, 7)))                                            # the stored fallback
    out.append(("bytes256", bytes(range(256))))
    out.append(("one_value", b"\x00" * 777))
    out.append(("no_match", bytes(random.Random(5).sample(range(256), 200))))          # every byte differs: an empty distance set
    out.append(("acgt", bytes(random.Random(6).choice(b"ACGT") for _ in range(5000))))
    return out


def scattered(items):
    """the pieces of `items` laid into one input array at odd offsets with gaps between them, not in order: (data, [(offset, length)])"""
    r = random.Random(11)
    order = list(range(len(items)))
    r.shuffle(order)
    data, where = bytearray(b"\xEE"), {}
    for i in order:
        if len(data) % 2 == 0:
            data += b"\xEE"
        where[i] = (len(data), len(items[i]))                                          # an odd offset
        data += items[i] + b"\xEE" * r.randint(1, 40)
    return np.frombuffer(bytes(data), np.uint8), [where[i] for i in range(len(items))]


def pieces_of(text):
    return [text[i:i + MAX_IN] for i in range(0, len(text), MAX_IN)]


@functools.lru_cache(maxsize=None)
def fastq_golden():
    return gzip.decompress(open(os.path.join(HERE, "golden", "cfg1_reads.fastq.gz"), "rb").read())


@functools.lru_cache(maxsize=None)
def fastq_5kb(n=6 * MAX_IN, seed=21):
    """5 kb reads: random bases, spread-out qualities, long nanopore-style ids"""
    g = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        length = int(g.integers(3000, 7000))
        rid = "%08x-%04x-%04x-%04x-%012x" % tuple(int(g.integers(0, 1 << b)) for b in (32, 16, 16, 16, 48))
        out += ("@%s runid=%040x sampleid=s1 read=%d ch=%d start_time=2024-03-01T12:%02d:%02dZ\n"
                % (rid, 0x1234567890ABCDEF1234, int(g.integers(1, 99999)), int(g.integers(1, 513)), int(g.integers(0, 60)), int(g.integers(0, 60)))).encode()
        out += np.frombuffer(b"ACGT", np.uint8)[g.integers(0, 4, length)].tobytes() + b"\n+\n"
        q = np.clip(np.rint(g.normal(20, 7, length)), 1, 50).astype(np.uint8) + 33
        out += q.tobytes() + b"\n"
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def fastq_150b(n=6 * MAX_IN, seed=22):
    """150 b reads with binned qualities (four values, in runs)"""
    g = np.random.default_rng(seed)
    bins = np.frombuffer(bytes([33 + 2, 33 + 12, 33 + 23, 33 + 37]), np.uint8)
    out, i = bytearray(), 0
    while len(out) < n:
        i += 1
        out += b"@SRR1234567.%d %d/1\n" % (i, i)
        out += np.frombuffer(b"ACGT", np.uint8)[g.integers(0, 4, 150)].tobytes() + b"\n+\n"
        change = g.random(150) < 0.1
        level = g.choice(4, 150, p=[0.02, 0.05, 0.13, 0.8])
        q = np.empty(150, np.int64)
        cur = 3
        for k in range(150):
            if change[k]:
                cur = level[k]
            q[k] = cur
        out += bins[q].tobytes() + b"\n"
    return bytes(out[:n])


def fixtures():
    return [("golden", fastq_golden), ("reads5kb", fastq_5kb), ("reads150b", fastq_150b)]


def zlib_raw_total(pieces, level):
    total = 0
    for p in pieces:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(p) + c.flush())
    return total


def inflate_raw(member, size):
    """what zlib's inflate makes of one raw deflate member that must decode to exactly `size` bytes and end with its last byte"""
    o = zlib.decompressobj(-15)
    out = o.decompress(member, size + 1)
    assert o.eof and not o.unused_data and len(out) == size
    return out


def parse_bgzf(blob):
    """the chain of BGZF blocks in `blob` as [(offset, bsize + 1, deflate bytes, crc32, isize)]; asserts the framing"""
    at, out = 0, []
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 10:at + 12] == b"\x06\x00" and blob[at + 12:at + 16] == b"BC\x02\x00", at
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        assert at + size <= len(blob)
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        out.append((at, size, blob[at + 18:at + size - 8], crc, isize))
        at += size
    return out


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
