#!/usr/bin/env python3
"""Regenerates foreign_members.bin: raw deflate members of a second writer, libdeflate (what current htslib builds usually deflate
BGZF with), for the inflate tests.  Needs the system's libdeflate.so.0; the tests read the file only and never load the library.

  texts     tests/deflate_cases.fastq_150b(20000) and fastq_5kb(20000), each at libdeflate levels 1 and 12
            (the order of tests/inflate_cases.FOREIGN_NAMES)
  format    a count, then for each member its input length, output length and zlib CRC-32 of the text as little-endian 32-bit words
            and its bytes

Every member is checked against zlib's inflate before it is written.
"""
import ctypes
import ctypes.util
import os
import struct
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import inflate_cases as ic  # noqa: E402


def main():
    lib = ctypes.CDLL(ctypes.util.find_library("deflate") or "libdeflate.so.0")
    lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    lib.libdeflate_deflate_compress_bound.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    texts = ic.foreign_texts()
    blob = struct.pack("<I", len(ic.FOREIGN_NAMES))
    for name in ic.FOREIGN_NAMES:
        text, level = texts[name.split("_")[0]], int(name.split("level")[1])
        c = lib.libdeflate_alloc_compressor(level)
        assert c
        room = lib.libdeflate_deflate_compress_bound(c, len(text))
        buf = ctypes.create_string_buffer(room)
        n = lib.libdeflate_deflate_compress(c, text, len(text), buf, room)
        lib.libdeflate_free_compressor(c)
        assert 0 < n <= room
        member = buf.raw[:n]
        assert ic.yardstick(member, len(text)) == (True, text), name
        blob += struct.pack("<III", n, len(text), zlib.crc32(text) & 0xFFFFFFFF) + member
        print("%-20s %6d -> %6d bytes" % (name, len(text), n))
    with open(os.path.join(HERE, "foreign_members.bin"), "wb") as f:
        f.write(blob)
    print("foreign_members.bin: %d bytes" % len(blob))


if __name__ == "__main__":
    main()
