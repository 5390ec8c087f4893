"""Cases for the record rule of the extract files (chn_extract_records_host, k_extract_records), shared by test_extract_records_cpu.py
and test_gpu_extract.py: texts with the descriptors of their records, and a plain Python restatement of the rule.  A text here need
not be FASTQ: a job names three ranges a record, wherever they lie."""
import itertools

import numpy as np

ID_LENGTHS = (0, 1, 15, 16, 17, 70)
SEQ_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 5000)
ACGT = b"ACGTacgt"
U = b"Uu"
IUPAC = b"NRYSWKMBDHVnryswkmbdhv"
LETTERS = ACGT + U + IUPAC

# host/fastx_reader.inc's CodeTable through "ACGTN"[code & 7]; a byte that is no letter maps to N (it cannot be in a read)
MAP = bytearray(b"N" * 256)
for _c in b"ACGT":
    MAP[_c] = _c
    MAP[_c + 32] = _c
MAP[ord("U")] = MAP[ord("u")] = ord("T")
MAP = bytes(MAP)


def py_records(text, d):
    """the rule, restated: '@' id '\\n' SEQ '\\n' '+' '\\n' qual '\\n' for every record of descriptor dict `d`"""
    text = bytes(text)
    out = []
    for i in range(len(d["id_offset"])):
        io, il, so, sl, qo, ql = (int(d[k][i]) for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset", "qual_length"))
        out.append(b"@" + text[io:io + il] + b"\n" + text[so:so + sl].translate(MAP) + b"\n+\n" + text[qo:qo + ql] + b"\n")
    return b"".join(out)


class Builder:
    """lays ranges into a text at chosen offsets from a 16-byte boundary, with filler between them that no record wants"""

    def __init__(self, seed):
        self.r = np.random.RandomState(seed)
        self.text = bytearray()
        self.d = {k: [] for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset", "qual_length")}

    def _place(self, data, off):
        at = (len(self.text) + 15) // 16 * 16 + off
        self.text += b"#" * (at - len(self.text)) + data
        return at

    def make_id(self, n):
        s = bytearray(self.r.randint(0x30, 0x7B, n).astype(np.uint8).tobytes())
        if n >= 3:
            s[n // 2] = 0x20  # a space inside
        return bytes(s)

    def make_seq(self, n, alphabet=LETTERS):
        return bytes(np.frombuffer(alphabet, np.uint8)[self.r.randint(0, len(alphabet), n)].tobytes())

    def make_qual(self, n):
        return self.r.randint(0x21, 0x7F, n).astype(np.uint8).tobytes()

    def add(self, rid, seq, qual, oi=0, os_=0, oq=0):
        for name, data, off in (("id", rid, oi), ("seq", seq, os_), ("qual", qual, oq)):
            self.d[name + "_offset"].append(self._place(data, off))
            self.d[name + "_length"].append(len(data))

    def done(self, end_pad=None):
        """(text, descriptors); the text ends with its last range unless end_pad bytes of filler follow"""
        if end_pad:
            self.text += b"#" * end_pad
        d = {k: np.array(v, np.uint64 if k.endswith("offset") else np.uint32) for k, v in self.d.items()}
        return bytes(self.text), d


def case_lengths():
    """every id length with every sequence length, the three source offsets walking through 0 .. 17 at different paces"""
    b = Builder(11)
    for k, (il, sl) in enumerate(itertools.product(ID_LENGTHS, SEQ_LENGTHS)):
        b.add(b.make_id(il), b.make_seq(sl), b.make_qual(sl), k % 18, (5 * k + 3) % 18, (7 * k + 11) % 18)
    return b.done()


def case_offsets():
    """source offsets 0 .. 17 for id, sequence and quality string independently (18^3 records of 17 + 17 + 17 bytes); the records'
    57 bytes walk the destination through every alignment"""
    b = Builder(12)
    rid, seq, qual = b.make_id(17), b.make_seq(17), b.make_qual(17)
    for oi, os_, oq in itertools.product(range(18), repeat=3):
        b.add(rid, seq, qual, oi, os_, oq)
    return b.done()


def case_letters():
    """every letter class, each letter at every position of a dword and of a 16-byte piece"""
    b = Builder(13)
    for shift in range(16):
        seq = bytes(LETTERS[(i + shift) % len(LETTERS)] for i in range(3 * len(LETTERS) + shift))
        b.add(b.make_id(9), seq, b.make_qual(len(seq)), shift, (shift * 3) % 18, 17 - shift)
    for cls in (ACGT[:4], ACGT[4:], U, IUPAC[:11], IUPAC[11:]):
        b.add(b"cls", b.make_seq(100, cls), b.make_qual(100), 1, 2, 3)
    return b.done()


def case_ragged_end():
    """the last quality string ends at a text_bytes that is no multiple of 16; so do, in turn, a sequence and an id"""
    out = []
    for which in range(3):
        b = Builder(14 + which)
        b.add(b.make_id(20), b.make_seq(40), b.make_qual(40), 3, 5, 7)
        parts = [("id", b.make_id(21)), ("seq", b.make_seq(37)), ("qual", b.make_qual(37))]
        parts = parts[which + 1:] + parts[:which + 1]  # the range that is laid last
        for name, data in parts:
            b.d[name + "_offset"].append(b._place(data, 9))
            b.d[name + "_length"].append(len(data))
        text, d = b.done()
        assert len(text) % 16 != 0
        out.append((text, d))
    return out


def crlf_fastq(n=40, seed=15):
    """a FASTQ text with \\r\\n line ends; the descriptors are chn_text_split_host's, which leave the \\r out"""
    b = Builder(seed)
    lines = []
    for i in range(n):
        sl = 1 + int(b.r.randint(0, 120))
        lines += [b"@" + b.make_id(5 + i % 30), b.make_seq(sl), b"+", b.make_qual(sl).replace(b"@", b"A").replace(b"+", b"B")]
    return b"\r\n".join(lines) + b"\r\n"


EMPTY = {k: np.zeros(0, np.uint64 if k.endswith("offset") else np.uint32)
         for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset", "qual_length")}


def args(d):
    return [d[k] for k in ("id_offset", "id_length", "seq_offset", "seq_length", "qual_offset", "qual_length")]
