"""A raw deflate (RFC 1951) writer that does what the test says, not what a compressor would choose, and a profiler that says which
decoder paths a member reaches.  Pure Python, nothing of the code under test: tests/inflate_cases.py builds its crafted members with
the writer and proves with the profiler that they hold what they were made for.  The expected bytes of a member always come from zlib
(inflate_cases.yardstick); `apply` below only sizes out_length.

    blocks   stored(data) | fixed(tokens) | dynamic(tokens, ll_lens, dd_lens, cl_symbols=None, hclen=19)
    tokens   an int 0 .. 255: a literal
             match(length, distance), or (MATCH, length symbol, length extra, distance symbol, distance extra)
             EOB: end of block (never added by the writer)
             (SYM, "ll" | "dd", symbol): that symbol's code alone;  (BITS, value, n): n bits, LSB first -- for the rejects
    cl_symbols   the code-length sequence as written: 0 .. 15, or (16, repeat), (17, repeat), (18, repeat)
"""
from tests.inflate_cases import BitWriter

MATCH, SYM, BITS = "match", "sym", "bits"
EOB = ("eob",)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [x for x in range(1, 14) for _ in range(2)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DD = [5] * 32
assert len(LEN_BASE) == len(LEN_EXTRA) == 29 and len(DIST_BASE) == len(DIST_EXTRA) == 30


# ---- blocks and tokens ---------------------------------------------------------------------------------------------------------------
def stored(data):
    return ("stored", bytes(data))


def fixed(tokens):
    return ("fixed", list(tokens))


def dynamic(tokens, ll_lens, dd_lens, cl_symbols=None, hclen=19):
    """ll_lens: 257 .. 288 code lengths (HLIT is their number), dd_lens: 1 .. 32 (HDIST); neither is checked for being a prefix code"""
    assert 257 <= len(ll_lens) <= 288 and 1 <= len(dd_lens) <= 32 and 4 <= hclen <= 19
    return ("dynamic", list(tokens), list(ll_lens), list(dd_lens), None if cl_symbols is None else list(cl_symbols), hclen)


def length_token(length):
    """(length symbol, extra) of a match length; 258 is symbol 285 (symbol 284 with extra 31 says 258 too: spell that token out)"""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, length - LEN_BASE[i]


def dist_token(dist):
    assert 1 <= dist <= 32768
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, dist - DIST_BASE[i]


def match(length, dist):
    return (MATCH,) + length_token(length) + dist_token(dist)


def match_length(tok):
    return LEN_BASE[tok[1] - 257] + tok[2]


def match_dist(tok):
    return DIST_BASE[tok[3]] + tok[4]


def apply(blocks, strict=True):
    """the writer's own idea of what `blocks` inflate to (raw tokens count for nothing): used to size out_length only.  A match that
    reaches in front of the text is an error, or with strict=False (members made to be rejected) counts as zero bytes"""
    text = bytearray()
    for b in blocks:
        if b[0] == "stored":
            text += b[1]
            continue
        for t in b[1]:
            if isinstance(t, int):
                text.append(t)
            elif t[0] == MATCH:
                length, dist = match_length(t), match_dist(t)
                assert dist <= len(text) or not strict, "the match reaches in front of the text"
                for _ in range(length):
                    text.append(text[-dist] if dist <= len(text) else 0)
    return text


# ---- codes ---------------------------------------------------------------------------------------------------------------------------
def canonical(lens):
    """{symbol: (code, bits)} of the canonical code of RFC 1951 3.2.2; the arithmetic is done whether or not the lengths are a prefix code"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def kraft(lens):
    """sum of 2^-length in units of 2^-15: 32 768 for a complete code"""
    return sum(1 << (15 - n) for n in lens if n)


def random_complete(r, symbols, max_len, n):
    """`n` code lengths: a random complete code of at most `max_len` bits over `symbols` (two or more), zero elsewhere: two 1-bit leaves,
    then a random leaf shorter than the limit is split until there is a leaf a symbol"""
    symbols = list(symbols)
    assert 2 <= len(symbols) <= (1 << max_len) and max_len <= 15 and max(symbols) < n
    leaves = [1, 1]
    while len(leaves) < len(symbols):
        short = [i for i, x in enumerate(leaves) if x < max_len]
        i = short[r.randrange(len(short))]
        leaves[i] += 1
        leaves.append(leaves[i])
    r.shuffle(leaves)
    lens = [0] * n
    for s, x in zip(symbols, leaves):
        lens[s] = x
    assert kraft(lens) == 32768
    return lens


def with_run(cl_symbols, start, code, rep):
    """`cl_symbols` (one length a symbol) with the entries [start, start + rep) replaced by one repeat code; checks that it says the same"""
    assert all(isinstance(x, int) for x in cl_symbols[start:start + rep]) and len(cl_symbols[start:start + rep]) == rep
    assert (code, 3 <= rep <= 6) == (16, True) or (code, 3 <= rep <= 10) == (17, True) or (code, 11 <= rep <= 138) == (18, True)
    want = cl_symbols[start - 1] if code == 16 else 0
    assert all(x == want for x in cl_symbols[start:start + rep]) and (code != 16 or (start > 0 and isinstance(want, int)))
    return cl_symbols[:start] + [(code, rep)] + cl_symbols[start + rep:]


def _cl_code_lengths(cl_symbols):
    """a complete code-length code (at most 5 bits) over the code-length symbols in use; zlib wants it complete, so a lone symbol gets company"""
    used = sorted({x if isinstance(x, int) else x[0] for x in cl_symbols})
    if len(used) < 2:
        used = sorted(used + [min(s for s in range(19) if s not in used)])
    k = 1
    while (1 << k) < len(used):
        k += 1
    shorter = (1 << k) - len(used)          # that many symbols get k - 1 bits, the rest k
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < shorter else k
    assert sum(1 << (7 - x) for x in lens if x) == 128
    return lens


# ---- the writer ----------------------------------------------------------------------------------------------------------------------
def _tokens(w, tokens, ll, dd):
    for t in tokens:
        if isinstance(t, int):
            w.code(*ll[t])
        elif t == EOB:
            w.code(*ll[256])
        elif t[0] == MATCH:
            _, ls, lx, ds, dx = t
            assert 0 <= lx < (1 << LEN_EXTRA[ls - 257]) and 0 <= dx < (1 << DIST_EXTRA[ds])
            w.code(*ll[ls]); w.field(lx, LEN_EXTRA[ls - 257])
            w.code(*dd[ds]); w.field(dx, DIST_EXTRA[ds])
        elif t[0] == SYM:
            w.code(*(ll if t[1] == "ll" else dd)[t[2]])
        elif t[0] == BITS:
            w.field(t[1], t[2])
        else:
            raise ValueError(t)


def write(blocks, starts=None):
    """the member: `blocks` in order, BFINAL on the last one.  starts: a list that receives each block's first bit position"""
    w = BitWriter()
    for k, b in enumerate(blocks):
        if starts is not None:
            starts.append(len(w.bits))
        w.field(1 if k == len(blocks) - 1 else 0, 1)
        if b[0] == "stored":
            w.field(0, 2)
            w.bits += [0] * (-len(w.bits) % 8)
            w.field(len(b[1]), 16); w.field(len(b[1]) ^ 0xFFFF, 16)
            for v in b[1]:
                w.field(v, 8)
        elif b[0] == "fixed":
            w.field(1, 2)
            _tokens(w, b[1], canonical(FIXED_LL), canonical(FIXED_DD))
        else:
            _, tokens, ll_lens, dd_lens, cl_symbols, hclen = b
            if cl_symbols is None:
                cl_symbols = ll_lens + dd_lens
            cl_lens = _cl_code_lengths(cl_symbols)
            assert all(cl_lens[s] == 0 for s in CL_ORDER[hclen:]), "hclen cuts a code-length code that is in use"
            cl = canonical(cl_lens)
            w.field(2, 2)
            w.field(len(ll_lens) - 257, 5); w.field(len(dd_lens) - 1, 5); w.field(hclen - 4, 4)
            for s in CL_ORDER[:hclen]:
                w.field(cl_lens[s], 3)
            for x in cl_symbols:
                if isinstance(x, int):
                    w.code(*cl[x])
                else:
                    s, rep = x
                    w.code(*cl[s])
                    w.field(rep - {16: 3, 17: 3, 18: 11}[s], {16: 2, 17: 3, 18: 7}[s])
            _tokens(w, tokens, canonical(ll_lens), canonical(dd_lens))
    return w.bytes()


# ---- the profiler --------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.data, self.at = data, 0

    def bit(self):
        if self.at >= 8 * len(self.data):
            raise ValueError("the member ends early")
        v = (self.data[self.at >> 3] >> (self.at & 7)) & 1
        self.at += 1
        return v

    def field(self, n):
        return sum(self.bit() << i for i in range(n))

    def symbol(self, table):
        """(symbol, bits) of the code at the cursor; table: {(code, bits): symbol}"""
        code = 0
        for n in range(1, 16):
            code = (code << 1) | self.bit()
            if (code, n) in table:
                return table[(code, n)], n
        raise ValueError("no such code")


def _decode_table(lens):
    return {v: s for s, v in canonical(lens).items()}


def profile(member):
    """what a valid member holds, found by a bit-by-bit decoder of its own (raises ValueError on a member that is not valid):
        blocks                 the block types in order: "stored" | "fixed" | "dynamic"
        block_bits             each block's first bit position
        stored_bits            the first bit position of each stored block's header
        len_symbols, dist_symbols      the length and distance symbols decoded from DYNAMIC tables
        ll_bits_in_match, dd_bits_in_match   the longest length-symbol code and distance code (dynamic tables) that a match used
        repeats_crossing       code-length repeat codes (16, 17, 18) that begin among the literal/length lengths and end among the distance lengths
        single_dist_sets, empty_dist_sets    dynamic blocks whose distance set is one 1-bit code / no code at all
        single_ll_sets         dynamic blocks whose literal/length set is one 1-bit code
        len_at_dist            {63: .., 64: .., 65: ..}: the largest match length met at that distance (0: none)
        out                    the text"""
    b = _Bits(member)
    p = dict(blocks=[], block_bits=[], stored_bits=[], len_symbols=set(), dist_symbols=set(), ll_bits_in_match=0, dd_bits_in_match=0,
             repeats_crossing=0, single_dist_sets=0, empty_dist_sets=0, single_ll_sets=0, len_at_dist={63: 0, 64: 0, 65: 0})
    out = bytearray()
    while True:
        p["block_bits"].append(b.at)
        final, kind = b.field(1), b.field(2)
        if kind == 3:
            raise ValueError("block type 3")
        p["blocks"].append(("stored", "fixed", "dynamic")[kind])
        if kind == 0:
            p["stored_bits"].append(b.at - 3)
            b.at += -b.at % 8
            n, c = b.field(16), b.field(16)
            if n ^ c != 0xFFFF or (b.at >> 3) + n > len(member):
                raise ValueError("stored block")
            out += member[b.at >> 3:(b.at >> 3) + n]
            b.at += 8 * n
        else:
            if kind == 1:
                ll, dd = _decode_table(FIXED_LL), _decode_table(FIXED_DD)
            else:
                hlit, hdist, hclen = b.field(5) + 257, b.field(5) + 1, b.field(4) + 4
                if hlit > 286 or hdist > 30:
                    raise ValueError("HLIT / HDIST")
                cl_lens = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl_lens[s] = b.field(3)
                cl, lens = _decode_table(cl_lens), []
                while len(lens) < hlit + hdist:
                    s, _ = b.symbol(cl)
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16 and not lens:
                        raise ValueError("repeat of nothing")
                    rep = b.field({16: 2, 17: 3, 18: 7}[s]) + {16: 3, 17: 3, 18: 11}[s]
                    if len(lens) < hlit < len(lens) + rep:
                        p["repeats_crossing"] += 1
                    lens += [lens[-1] if s == 16 else 0] * rep
                if len(lens) > hlit + hdist or lens[256] == 0:
                    raise ValueError("code lengths")
                ll_lens, dd_lens = lens[:hlit], lens[hlit:]
                for name, x in (("ll", ll_lens), ("dd", dd_lens)):
                    used = [n for n in x if n]
                    if used == [1]:
                        p["single_ll_sets" if name == "ll" else "single_dist_sets"] += 1
                    elif not used and name == "dd":
                        p["empty_dist_sets"] += 1
                    elif kraft(x) != 32768:
                        raise ValueError("not a complete code")
                ll, dd = _decode_table(ll_lens), _decode_table(dd_lens)
            while True:
                s, n = b.symbol(ll)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise ValueError("length symbol")
                length = LEN_BASE[s - 257] + b.field(LEN_EXTRA[s - 257])
                d, dn = b.symbol(dd)
                if d > 29:
                    raise ValueError("distance symbol")
                dist = DIST_BASE[d] + b.field(DIST_EXTRA[d])
                if dist > len(out):
                    raise ValueError("distance")
                if kind == 2:
                    p["len_symbols"].add(s); p["dist_symbols"].add(d)
                    p["ll_bits_in_match"] = max(p["ll_bits_in_match"], n); p["dd_bits_in_match"] = max(p["dd_bits_in_match"], dn)
                if dist in p["len_at_dist"]:
                    p["len_at_dist"][dist] = max(p["len_at_dist"][dist], length)
                for _ in range(length):
                    out.append(out[-dist])
        if final:
            break
    p["out"] = bytes(out)
    return p
