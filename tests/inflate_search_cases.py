"""Cases for chn_inflate_stream_search_host (the block-start search of a one-stream .gz round) and an
independent restatement of its rule.  Pure Python and numpy, nothing of the code under test.

THE RULE (include/charon_hip.h).  find(data, from, to) is the first bit position p in [from, to) -- LSB first, from bit 0 -- with
  R0  (p >> 3) + 8 <= len(data), and with at = p + 17: (at >> 3) + 9 <= len(data)
  R1  the 3 bits at p are 4 (BFINAL 0, BTYPE 2), HLIT field <= 29, HDIST field <= 29
  R2  of the HCLEN + 4 three-bit lengths at p + 17: sum of 128 >> l over the non-zero l is 128
  R3  the dynamic header parses (zlib's rules)
  R4  the block decodes to end-of-block or until >= 32 768 symbols are out (count looked at in front of every literal/length code, a
      match counts as its length, nothing is read once the count is reached); literals are text; codes are valid; no bit behind the
      input is consumed; no distance check
  R5  >= 32 symbols
  R6  behind an end-of-block: a block header that parses (stored with LEN == ~NLEN | fixed | dynamic as R3), BFINAL either way
The restatement reads bit by bit from a list of bits and decodes canonical codes through a dictionary; R0 - R2 are evaluated for all
positions at once with numpy (prefilter), the rest position by position (trial), both cached per input.

A case: name, data, ranges [(from, to)], and `true` -- per range the position the writer knows the answer to be (a block start it
wrote), None where it knows there is none, or ANY where only the restatement says.  expected(case) is the restatement's answer; check()
compares a result with it and asserts that the restatement agrees with `true`.

R0 never decides alone: the shortest block that passes R1 - R6 takes 116 bits (hclen 16, a code-length code of two 1-bit codes, four
2-bit literal/length codes, one literal, one match, end-of-block, three bits of a follower), and R0 asks for at most 96 from the
position's byte on.  So "the R0 tests fail by one byte" and "the input ends inside the block" cannot be told apart from outside: the
input-end cases cut a block at the last byte its trial needs (found), one byte short of it (refuted), and where R0 fails by one byte
and by none (both refuted: the block is cut as well)."""
import functools
import random
import zlib

import numpy as np

from tests import deflate_writer as dw
from tests import inflate_stream_cases as isc

ANY = "any"
EOB = dw.EOB
LIMIT, LEAST = 32768, 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
TEXT = frozenset([9, 10, 13] + list(range(32, 127)))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
class Refuted(Exception):
    pass


class Reader:
    def __init__(self, bits, at):
        self.bits, self.at, self.end = bits, at, len(bits)

    def field(self, n):
        if self.at + n > self.end:
            raise Refuted("the input ends")
        v = 0
        for i in range(n):
            v |= self.bits[self.at + i] << i
        self.at += n
        return v

    def symbol(self, codes):
        code = 0
        for n in range(1, 16):
            if self.at >= self.end:
                raise Refuted("the input ends")
            code = (code << 1) | self.bits[self.at]
            self.at += 1
            s = codes.get((n, code))
            if s is not None:
                return s
        raise Refuted("no such code")


def codes_of(lens, may_be_single, may_be_empty):
    """{(bits, code): symbol} of a set zlib accepts: complete, or -- where allowed -- one code of one bit, or none at all"""
    used = [n for n in lens if n]
    if not used:
        if may_be_empty:
            return {}
        raise Refuted("no code")
    space = sum(1 << (15 - n) for n in used)
    if space > 32768:
        raise Refuted("over-subscribed")
    if space < 32768 and not (may_be_single and used == [1]):
        raise Refuted("incomplete")
    count = [0] * 16
    for n in used:
        count[n] += 1
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[(n, nxt[n])] = s
            nxt[n] += 1
    return out


def dynamic_header(r):
    """the reader stands behind the three header bits"""
    hlit, hdist, hclen = r.field(5) + 257, r.field(5) + 1, r.field(4) + 4
    if hlit > 286 or hdist > 30:
        raise Refuted("HLIT / HDIST")
    cl = [0] * 19
    for s in CL_ORDER[:hclen]:
        cl[s] = r.field(3)
    clc = codes_of(cl, False, False)
    lens = []
    while len(lens) < hlit + hdist:
        s = r.symbol(clc)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Refuted("repeat of nothing")
            rep, val = 3 + r.field(2), lens[-1]
        elif s == 17:
            rep, val = 3 + r.field(3), 0
        else:
            rep, val = 11 + r.field(7), 0
        if len(lens) + rep > hlit + hdist:
            raise Refuted("repeat past the end")
        lens += [val] * rep
    if lens[256] == 0:
        raise Refuted("no end-of-block code")
    return codes_of(lens[:hlit], True, False), codes_of(lens[hlit:], True, True)


def trial(bits, p):
    """R3 - R6 at position p: True, or the reason it is refuted"""
    r = Reader(bits, p + 3)
    try:
        ll, dd = dynamic_header(r)
        n, ended = 0, False
        while n < LIMIT:
            s = r.symbol(ll)
            if s < 256:
                if s not in TEXT:
                    raise Refuted("not text")
                n += 1
            elif s == 256:
                ended = True
                break
            elif s > 285:
                raise Refuted("length symbol")
            else:
                length = LBASE[s - 257] + r.field(LEXTRA[s - 257])
                d = r.symbol(dd)
                if d > 29:
                    raise Refuted("distance symbol")
                r.field(DEXTRA[d])
                n += length
        if n < LEAST:
            raise Refuted("fewer than 32 symbols")
        if ended:
            kind = r.field(3) >> 1
            if kind == 3:
                raise Refuted("block type 3")
            if kind == 2:
                dynamic_header(r)
            elif kind == 0:
                r.at += -r.at % 8
                a, b = r.field(16), r.field(16)
                if a ^ b != 0xFFFF:
                    raise Refuted("LEN / NLEN")
        return True
    except Refuted as e:
        return str(e)


class Searcher:
    """the restatement over one input: R0 - R2 for every position at once, trials on demand and remembered"""

    def __init__(self, data):
        self.n = len(data)
        b = np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little") if data else np.zeros(0, np.uint8)
        self.bits = b.tolist()
        nb, pad = 8 * self.n, np.concatenate([b, np.zeros(96, np.uint8)]).astype(np.int64)

        def field(off, width):
            return sum(pad[off + k:off + k + nb] << k for k in range(width))
        p = np.arange(nb, dtype=np.int64)
        ok = ((p >> 3) + 8 <= self.n) & (((p + 17) >> 3) + 9 <= self.n)
        ok &= (field(0, 3) == 4) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
        self.r1 = np.flatnonzero(ok)
        ncode, kraft = field(13, 4) + 4, np.zeros(nb, np.int64)
        for i in range(19):
            l = field(17 + 3 * i, 3)
            kraft += np.where((i < ncode) & (l > 0), 128 >> l, 0)
        self.r2 = np.flatnonzero(ok & (kraft == 128))
        self.done = {}

    def passes(self, p):
        if p not in self.done:
            self.done[p] = trial(self.bits, p)
        return self.done[p] is True

    def parses(self, p):
        """R3 alone at a survivor of R2 (for the count the filter-coverage test prints)"""
        try:
            dynamic_header(Reader(self.bits, p + 3))
            return True
        except Refuted:
            return False

    def find(self, frm, to):
        lo, hi = np.searchsorted(self.r2, frm), np.searchsorted(self.r2, to)
        for p in self.r2[lo:hi].tolist():
            if self.passes(p):
                return p
        return None


_searchers = {}


def searcher(data):
    data = bytes(data)
    if data not in _searchers:
        _searchers[data] = Searcher(data)
    return _searchers[data]


def expected(c):
    s = searcher(c["data"])
    return [s.find(f, t) for f, t in c["ranges"]]


def check(found, c):
    """found: the list api.inflate_search_host returns for the case's ranges"""
    want = expected(c)
    for k, t in enumerate(c["true"]):
        if t is not ANY:
            assert want[k] == t, (c["name"], "the restatement and the writer disagree", k, c["ranges"][k], want[k], t)
    assert list(found) == want, (c["name"], [(r, f, w) for r, f, w in zip(c["ranges"], found, want) if f != w][:5])


def run(fn, c):
    """fn: api.inflate_search_host"""
    return fn(c["data"], [f for f, _ in c["ranges"]], [t for _, t in c["ranges"]])


def make(name, data, ranges, true=None):
    return dict(name=name, data=bytes(data), ranges=[(int(f), int(t)) for f, t in ranges], true=list(true) if true is not None else [ANY] * len(ranges))


# ---- building streams bit by bit ---------------------------------------------------------------------------------------------------
TEXT_ALPHABET = b"ACGTN@+:#FF,\n 0123456789"
TAIL = [0] * 256  # zero bits: no position among them passes R1, and every trial in front of them has input enough


def block_bits(block, final=False):
    """the bits of one writer block alone, written at bit 0 (a stored block would be aligned for that position: not for these)"""
    assert block[0] != "stored"
    starts = []
    data = dw.write([block] if final else [block, dw.fixed([EOB])], starts)
    n = 8 * len(data) if final else starts[1]
    bits = isc._bits(data, n)
    if final:  # the writer pads the last byte
        bits = bits[:_bit_length(block)]
    return bits


def _bit_length(block):
    starts = []
    dw.write([block, dw.fixed([EOB])], starts)
    return starts[1]


def text_lens(r, extra_literals=(), lengths=(), max_len=9):
    """literal/length code lengths (286 of them) of a random complete code over the text alphabet, end-of-block, and what is asked for"""
    syms = sorted(set(TEXT_ALPHABET) | set(extra_literals) | {256} | set(lengths))
    return dw.random_complete(r, syms, max_len, 286)


def dist_lens(r, symbols=(0, 3, 8, 29)):
    return dw.random_complete(r, list(symbols), 5, 30)


def text_tokens(r, n):
    return [r.choice(TEXT_ALPHABET) for _ in range(n)]


def text_block(r, n, **kw):
    """a dynamic block of n text literals and end-of-block"""
    return dw.dynamic(text_tokens(r, n) + [EOB], text_lens(r, **kw), dist_lens(r))


class Bits:
    """a stream put together from pieces, position by position"""

    def __init__(self):
        self.bits = []

    def at(self):
        return len(self.bits)

    def add(self, bits):
        at = len(self.bits)
        self.bits += list(bits)
        return at

    def zeros(self, n):
        return self.add([0] * n)

    def align(self):
        return self.add([0] * (-len(self.bits) % 8))

    def data(self):
        return isc._pack(self.bits)


def whole(data):
    return (0, 8 * len(data))


# ---- alignment and range ends ---------------------------------------------------------------------------------------------------------
def alignment_cases():
    """a dynamic text block at each of the eight bit alignments behind a stored block (a fixed block of k nine-bit literals between
    them shifts it), and the ranges around its first bit"""
    out, seen = [], set()
    for k in range(8):
        r = random.Random(100 + k)
        blocks = [dw.stored(bytes(40)), dw.fixed([144 + k] * k + [EOB]), text_block(r, 60 + k), text_block(r, 45), dw.fixed([EOB])]
        starts = []
        data = dw.write(blocks, starts) + bytes(32)
        s, nxt, end = starts[2], starts[3], 8 * len(data)
        seen.add(s % 8)
        out.append(make("align_%d" % (s % 8), data, [(0, end), (s, end), (s + 1, end), (0, s), (s, s + 1), (s, s), (s + 1, s + 1), (nxt, nxt + 1), (s + 1, nxt)],
                        [s, s, nxt, None, s, None, None, nxt, None]))
    assert seen == set(range(8))
    return out


# ---- decoys ------------------------------------------------------------------------------------------------------------------------
def _decoy_stream(name, decoy_bits, seed, why, follower=None):
    """zeros | the decoy | follower(stream) bits: an empty fixed block unless the follower is what is wrong | zeros | a true block |
    an empty final fixed block | zeros.  The answer over the whole input is the true block's start, or the decoy's where it is none
    (why = None).  why: "r1" / "r2" -- the decoy falls to that filter -- or what the restatement's trial says of it, so that a decoy
    that falls for another reason than the one it was made for is noticed (check_decoy)"""
    r = random.Random(seed)
    b = Bits()
    b.zeros(64 + seed % 8)
    d = b.add(decoy_bits)
    b.add(follower(b) if follower else block_bits(dw.fixed([EOB])))
    b.zeros(40)
    t = b.add(block_bits(text_block(r, 50)))
    b.add(block_bits(dw.fixed([EOB]), final=True))
    b.add(TAIL)
    data = b.data()
    end = 8 * len(data)
    c = make(name, data, [(0, end), (d, d + 1), (d + 1, end), (t, t + 1)], [d if why is None else t, d if why is None else None, t, t])
    c["decoy"], c["why"] = d, why
    return c


def check_decoy(c):
    """the decoy of a decoy case falls to the rule it was made for, by the restatement"""
    s, d, why = searcher(c["data"]), c["decoy"], c["why"]
    in_r1, in_r2 = d in set(s.r1.tolist()), d in set(s.r2.tolist())
    if why == "r1":
        assert not in_r1, c["name"]
    elif why == "r2":
        assert in_r1 and not in_r2, c["name"]
    else:
        assert in_r2, c["name"]
        got = trial(s.bits, d)
        assert got == (True if why is None else why), (c["name"], got, why)


def _raw_header(cl_len_fields, hlit=29, hdist=29, bfinal=0):
    w = isc.ic.BitWriter()
    w.field(bfinal, 1); w.field(2, 2); w.field(hlit, 5); w.field(hdist, 5); w.field(len(cl_len_fields) - 4, 4)
    for v in cl_len_fields:
        w.field(v, 3)
    return w.bits + [0] * 64


def _failing_dynamic(r):
    """a dynamic header that passes R1 and R2 and fails in the walk (a repeat of nothing)"""
    ll, dd = text_lens(r), dist_lens(r)
    return block_bits(dw.dynamic([], ll, dd, cl_symbols=[(16, 3)] + (ll + dd)[3:]))


def decoy_cases():
    out = []
    r = random.Random(7)
    # R1 passes, R2 fails: nineteen code-length-code lengths of 1
    out.append(_decoy_stream("decoy_r2_kraft", _raw_header([1] * 19), 1, "r2"))
    out.append(_decoy_stream("decoy_r2_kraft_short", _raw_header([2, 2, 2, 0, 3]), 2, "r2"))
    # R2 passes, the code-length walk fails
    ll, dd = text_lens(r), dist_lens(r)
    seq = ll + dd
    out.append(_decoy_stream("decoy_repeat_at_0", block_bits(dw.dynamic(text_tokens(r, 40), ll, dd, cl_symbols=[(16, 3)] + seq[3:])), 3, "repeat of nothing"))
    out.append(_decoy_stream("decoy_repeat_past_end", block_bits(dw.dynamic(text_tokens(r, 40), ll, dd, cl_symbols=seq[:-2] + [(18, 11)])), 4, "repeat past the end"))
    no_eob = dw.random_complete(r, sorted(set(TEXT_ALPHABET)), 9, 286)
    out.append(_decoy_stream("decoy_no_eob", block_bits(dw.dynamic(text_tokens(r, 40), no_eob, dd)), 5, "no end-of-block code"))
    over = list(ll)
    over[ord("!")] = 1
    assert dw.kraft(over) > 32768
    out.append(_decoy_stream("decoy_ll_oversubscribed", block_bits(dw.dynamic([(dw.BITS, 0x2A5, 10)] * 8, over, dd)), 6, "over-subscribed"))
    short_dd = [2, 2] + [0] * 28
    out.append(_decoy_stream("decoy_dd_incomplete", block_bits(dw.dynamic(text_tokens(r, 40) + [EOB], ll, short_dd)), 7, "incomplete"))
    # the header parses, a literal is not text: as the first symbol and as the 40th
    for v in (0x00, 0x7F, 0x80):
        lens = text_lens(r, extra_literals=[v])
        for where in (0, 39):
            toks = text_tokens(r, 60)
            toks[where] = v
            out.append(_decoy_stream("decoy_literal_%02x_at_%d" % (v, where), block_bits(dw.dynamic(toks + [EOB], lens, dd)), 8 + where + v, "not text"))
    # 31 symbols are too few, 32 are enough
    out.append(_decoy_stream("decoy_31_symbols", block_bits(text_block(r, 31)), 9, "fewer than 32 symbols"))
    out.append(_decoy_stream("found_32_symbols", block_bits(text_block(r, 32)), 10, None))
    # 29 literals and a match of three: 32 symbols; of a match of two fewer there is none, so 28 literals and a match of three: 31
    lens_m = text_lens(r, lengths=[257])
    out.append(_decoy_stream("found_29_and_match_3", block_bits(dw.dynamic(text_tokens(r, 29) + [dw.match(3, 1), EOB], lens_m, dist_lens(r))), 11, None))
    out.append(_decoy_stream("decoy_28_and_match_3", block_bits(dw.dynamic(text_tokens(r, 28) + [dw.match(3, 1), EOB], lens_m, dist_lens(r))), 12, "fewer than 32 symbols"))
    # a good block with BFINAL = 1
    fin = block_bits(text_block(r, 50))
    fin[0] = 1
    out.append(_decoy_stream("decoy_bfinal", fin, 13, "r1"))
    # end-of-block, then no block
    good = block_bits(text_block(r, 50))
    out.append(_decoy_stream("decoy_then_type_3", good + [0, 1, 1], 14, "block type 3"))
    out.append(_decoy_stream("decoy_then_final_type_3", good + [1, 1, 1], 15, "block type 3"))

    def bad_stored(b):
        return [0, 0, 0] + [0] * (-(b.at() + 3) % 8) + isc._field(5, 16) + isc._field(5 ^ 0xFFFF ^ 0x0100, 16)
    out.append(_decoy_stream("decoy_then_bad_stored", good, 16, "LEN / NLEN", follower=bad_stored))
    out.append(_decoy_stream("decoy_then_bad_stored_b", good, 21, "LEN / NLEN", follower=bad_stored))  # (another alignment of the follower)
    out.append(_decoy_stream("decoy_then_bad_dynamic", good + _failing_dynamic(r), 17, "repeat of nothing"))
    out.append(_decoy_stream("decoy_then_kraft_dynamic", good + _raw_header([1] * 19), 18, "over-subscribed"))
    return out


# ---- followers that are accepted -----------------------------------------------------------------------------------------------------
def follower_cases():
    out = []
    r = random.Random(17)
    for name, follower, final in (("stored", dw.stored(b"\x00\xff" * 20), False), ("fixed", dw.fixed(text_tokens(r, 10) + [EOB]), False),
                                  ("dynamic", text_block(r, 5), False), ("final_dynamic", text_block(r, 5), True),
                                  ("final_stored", dw.stored(b""), True), ("final_fixed", dw.fixed([EOB]), True)):
        for lead in (0, 3, 5):  # where the follower's header falls in its byte
            starts = []
            blocks = [dw.stored(bytes(20)), dw.fixed([144] * lead + [EOB]), text_block(r, 40 + lead), follower] + ([] if final else [dw.fixed([EOB])])
            data = dw.write(blocks, starts) + bytes(32)
            s = starts[2]
            out.append(make("follower_%s_%d" % (name, lead), data, [whole(data), (s, s + 1)], [s, s]))
    return out


def distance_set_cases():
    """an all-literal block whose distance set is a single 1-bit code / empty (zlib accepts both), and a first symbol that is a match of
    distance 32 768 (the search has no distance rule)"""
    out = []
    r = random.Random(19)
    for name, dd in (("single", [1]), ("single_of_30", [0] * 29 + [1]), ("empty", [0]), ("empty_of_30", [0] * 30)):
        starts = []
        data = dw.write([dw.stored(bytes(24)), dw.dynamic(text_tokens(r, 64) + [EOB], text_lens(r), dd), dw.fixed([EOB])], starts) + bytes(32)
        out.append(make("dist_set_" + name, data, [whole(data)], [starts[1]]))
    for name, toks in (("first", [dw.match(40, 32768)] + text_tokens(r, 3)), ("only", [dw.match(32, 32768)]), ("short", [dw.match(31, 32768)])):
        starts = []
        blk = dw.dynamic(toks + [EOB], text_lens(r, lengths=[dw.length_token(dw.match_length(toks[0]))[0]]), dist_lens(r))
        data = dw.write([dw.stored(bytes(24)), blk, text_block(r, 40), dw.fixed([EOB])], starts) + bytes(32)
        out.append(make("far_match_" + name, data, [whole(data)], [starts[2] if name == "short" else starts[1]]))
    return out


# ---- the limit of 32 768 symbols -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def limit_cases():
    out = []
    r = random.Random(23)

    def stream(name, toks, lens, dd, found):
        starts = []
        data = dw.write([dw.stored(bytes(24)), dw.dynamic(toks + [EOB], lens, dd), text_block(r, 40), dw.fixed([EOB])], starts) + bytes(32)
        out.append(make(name, data, [whole(data), (starts[1], starts[1] + 1)], [starts[1] if found else starts[2], starts[1] if found else None]))
    lens0 = text_lens(r, extra_literals=[0])
    for name, at, found in (("nontext_at_32768", 32768, True), ("nontext_at_32767", 32767, False), ("nontext_at_32769", 32769, True)):
        toks = text_tokens(r, 40000)
        toks[at] = 0
        stream("limit_" + name, toks, lens0, dist_lens(r), found)
    # an invalid code there: a length code in front of an empty distance set
    lens1 = text_lens(r, lengths=[257])
    for name, at, found in (("invalid_at_32768", 32768, True), ("invalid_at_32767", 32767, False)):
        toks = text_tokens(r, 40000)
        toks[at] = (dw.SYM, "ll", 257)
        stream("limit_" + name, toks, lens1, [0], found)
    # a match of 258 from symbol 32 600 on crosses the limit; noise behind it
    noise = [(dw.BITS, r.getrandbits(16), 16) for _ in range(300)]
    lens2 = text_lens(r, lengths=[285])
    stream("limit_match_crosses", text_tokens(r, 32600) + [dw.match(258, 100)] + noise, lens2, dist_lens(r, (0, 3, 12, 13)), True)
    # ... and a match that ends exactly on it, with a non-text literal behind
    lens3 = text_lens(r, extra_literals=[0], lengths=[285])
    stream("limit_match_ends_on_it", text_tokens(r, 32768 - 258) + [dw.match(258, 100), 0] + text_tokens(r, 50), lens3, dist_lens(r, (0, 3, 12, 13)), True)
    stream("limit_match_ends_before_it", text_tokens(r, 32767 - 258) + [dw.match(258, 100), 0] + text_tokens(r, 50), lens3, dist_lens(r, (0, 3, 12, 13)), False)
    return out


# ---- never found -----------------------------------------------------------------------------------------------------------------------
def never_cases():
    out = []
    for name, level, strategy in (("level0", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED)):
        data = isc.zstream("small", level, strategy, 20000)[0]
        end = 8 * len(data)
        cuts = list(range(0, end, 8 * 4096 + 3)) + [end]
        out.append(make("never_" + name, data, [(0, end)] + list(zip(cuts[:-1], cuts[1:])), [None] * len(cuts)))
    return out


# ---- where the input ends ----------------------------------------------------------------------------------------------------------------
def input_end_cases():
    out = []
    r = random.Random(29)
    for lead in (0, 1, 7):
        b = Bits()
        b.zeros(64 + lead)
        s = b.add(block_bits(text_block(r, 40)))
        last = b.add([1, 1, 0]) + 3  # a final fixed block's header: the last bits the trial reads
        b.add([0] * 7 + TAIL)
        data = b.data()
        need = (last + 7) // 8  # bytes the trial needs
        assert need > ((s + 17) >> 3) + 9  # (see the module's docstring: R0 never decides alone)
        out.append(make("input_end_exact_%d" % lead, data[:need], [(0, 8 * need)], [s]))
        out.append(make("input_end_short_%d" % lead, data[:need - 1], [(0, 8 * (need - 1))], [None]))
        out.append(make("input_end_long_%d" % lead, data[:need + 1], [(0, 8 * (need + 1))], [s]))
        r0 = ((s + 17) >> 3) + 9
        for k in (r0 - 1, r0, (s >> 3) + 8, (s >> 3) + 7, (s >> 3) + 1):
            out.append(make("input_end_r0_%d_%d" % (lead, k), data[:k], [(0, 8 * k), (s, min(s + 1, 8 * k))], [None, None]))
        # the block cut in its header, in its code lengths, in its symbols
        for k in sorted({need - 2, need - 10, (s >> 3) + 14, (s >> 3) + 20}):
            out.append(make("input_end_inside_%d_%d" % (lead, k), data[:k], [(0, 8 * k)], [None]))
    out.append(make("input_empty", b"", [(0, 0)], [None]))
    out.append(make("input_tiny", b"\x04" * 7, [(0, 56), (3, 9)], [None, None]))
    return out


# ---- the filters, over noise ---------------------------------------------------------------------------------------------------------
NOISE_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def noise(seed):
    return random.Random(seed).randbytes(65536)


def noise_cases():
    out = []
    for seed in NOISE_SEEDS:
        data = noise(seed)
        end = 8 * len(data)
        r = random.Random(1000 + seed)
        cuts = [0]
        while len(cuts) < 97:  # 97 ranges of odd bit lengths; the last one ends one bit short of the end (96 odd lengths are even)
            cuts.append(cuts[-1] + 2 * r.randrange(end // 97 // 2 - 400, end // 97 // 2) + 1)
        cuts.append(end - 1)
        assert cuts[-2] < end - 1 and len(cuts) == 98 and all((b - a) % 2 == 1 for a, b in zip(cuts[:-1], cuts[1:]))
        out.append(make("noise_%d_one" % seed, data, [(0, end)]))
        out.append(make("noise_%d_97" % seed, data, list(zip(cuts[:-1], cuts[1:]))))
    return out


@functools.lru_cache(maxsize=None)
def planted(seed):
    """(data, header positions, block positions): noise(seed) with 64 pieces written over it, 1 KiB and a byte apart and at bit k % 8
    of their byte, so that in a search from bit 0 every lane of a window of 64 bytes and every bit offset gets one: 56 dynamic headers
    that parse (R3) with the noise going on behind them, and 8 whole text blocks with an empty fixed block behind them.
    Noise alone does not exercise R3's passing side: of the 1.4 million survivors of R2 in the noise of seeds 4 .. 5999 not one parses."""
    r = random.Random(2000 + seed)
    bits = isc._bits(noise(seed), 8 * 65536)
    headers, blocks = [], []
    for k in range(64):
        at = 8 * (1025 * k + 300) + k % 8
        if k % 8 == 5:
            piece = block_bits(text_block(r, 40 + k)) + block_bits(dw.fixed([EOB]))
            blocks.append(at)
        else:
            piece = block_bits(dw.dynamic([], text_lens(r, extra_literals=list(range(9)) + list(range(127, 160))), dist_lens(r)))  # (the noise behind it soon decodes to a byte that is not text)
            headers.append(at)
        bits[at:at + len(piece)] = piece
    assert len(bits) == 8 * 65536 and len({(p >> 3) % 64 for p in headers + blocks}) == 64
    return isc._pack(bits), headers, blocks


def planted_cases():
    out = []
    for seed in NOISE_SEEDS:
        data, headers, blocks = planted(seed)
        end = 8 * len(data)
        out.append(make("planted_%d_one" % seed, data, [(0, end)] + [(b + 1, end) for b in blocks] + [(b, b + 1) for b in blocks], [ANY] * 9 + blocks))
        out.append(make("planted_%d_97" % seed, data, noise_cases()[2 * NOISE_SEEDS.index(seed) + 1]["ranges"]))
    return out


def noise_census():
    """[(name, positions that pass R0 - R1, ... R2, ... R3)] of the noise and of the noise with pieces planted"""
    out = []
    for seed in NOISE_SEEDS:
        for name, data in (("noise_%d" % seed, noise(seed)), ("planted_%d" % seed, planted(seed)[0])):
            s = searcher(data)
            out.append((name, len(s.r1), len(s.r2), sum(1 for p in s.r2.tolist() if s.parses(p))))
    return out


# ---- zlib's streams ----------------------------------------------------------------------------------------------------------------------
def _ranges(end, step_bits):
    cuts = list(range(0, end, step_bits)) + [end]
    return list(zip(cuts[:-1], cuts[1:]))


@functools.lru_cache(maxsize=None)
def real_cases():
    out = []
    for name, level in (("l1", 1), ("l6", 6), ("l9", 9)):
        data = isc.zstream("fastq", level, zlib.Z_DEFAULT_STRATEGY, 40000)[0]
        end = 8 * len(data)
        out.append(make("real_%s_4k" % name, data, _ranges(end, 8 * 4096)))
        out.append(make("real_%s_20k" % name, data, _ranges(end, 8 * 20480)))
    return out


@functools.lru_cache(maxsize=None)
def flushed_stream():
    """a level-6 FASTQ stream with a sync flush every 50 records: (data, [bit position of the block behind each flush])"""
    text = isc.fastq()
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    out, recs, at, starts = b"", 0, 0, []
    lines = text.split(b"\n")
    for k in range(0, len(lines) - 1, 4 * 50):
        out += c.compress(b"\n".join(lines[k:k + 200]) + b"\n")
        out += c.flush(zlib.Z_SYNC_FLUSH)
        starts.append(8 * len(out))
    return out + c.flush(), starts[:-1]


@functools.lru_cache(maxsize=None)
def cursor_case():
    """600 ranges -- more than the grid of two wavefronts a CU -- in no order and overlapping, over the flushed stream"""
    data, starts = flushed_stream()
    end = 8 * len(data)
    r = random.Random(37)
    ranges, true = [], []
    for s in starts[:100]:  # ranges that begin on a flush point find it (it is a dynamic block of 50 records)
        ranges.append((s, min(end, s + 20000)))
        true.append(s)
    while len(ranges) < 600:
        f = r.randrange(end)
        ranges.append((f, min(end, f + r.randrange(1, 60000))))
        true.append(ANY)
    order = list(range(600))
    r.shuffle(order)
    return make("cursor_600", data, [ranges[i] for i in order], [true[i] for i in order])


def crafted_cases():
    return alignment_cases() + decoy_cases() + follower_cases() + distance_set_cases() + never_cases() + input_end_cases()


def all_cases():
    return crafted_cases() + list(limit_cases()) + noise_cases() + planted_cases() + list(real_cases()) + [cursor_case()]


# ---- jobs that are refused -----------------------------------------------------------------------------------------------------------
def invalid_jobs(api):
    """[(name, job, arrays, what chn_last_error() names)]: each is CHN_E_INVALID and leaves found_bit as it was"""
    data = noise(1)[:4096]
    end = 8 * len(data)
    out = []

    def job(name, says, frm=(0, 100, 200), to=(50, 150, end), edit=None):
        j, a = api.inflate_search_job(data, list(frm), list(to))
        if edit:
            edit(j)
        out.append((name, j, a, says))
    job("struct_size", "struct_size", edit=lambda j: setattr(j, "struct_size", j.struct_size - 8))
    job("flag", "flag", edit=lambda j: setattr(j, "flags", 1))
    job("too_many", "n_ranges", edit=lambda j: setattr(j, "n_ranges", api.INFLATE_STREAM_MAX_CHUNKS + 1))
    job("null_from", "NULL", edit=lambda j: setattr(j, "from_bit", None))
    job("null_to", "NULL", edit=lambda j: setattr(j, "to_bit", None))
    job("null_found", "NULL", edit=lambda j: setattr(j, "found_bit", None))
    job("null_in", "NULL", edit=lambda j: setattr(j, "in_", None))
    job("from_behind_to", "range 1", frm=(0, 151, 200))
    job("to_beyond_in", "range 2", to=(50, 150, end + 1))
    return out
