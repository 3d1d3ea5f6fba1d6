"""Inputs of the gzip tests (tests/test_gunzip_host.py, tests/test_gpu_gunzip.py): single-stream gzip files of every kind the parallel inflate has a path for,
each seeded, each with the text that Python's gzip / zlib gives for it.  Test infrastructure only."""
import functools
import gzip
import random
import struct
import zlib

from tests import bgzf_util as bu

CHUNKS = (8 << 10, 32 << 10, 0)                                     # compressed bytes per chunk: most chunks without a start, a start in every chunk, the default


def gz_member(text, level=6, strategy="default", flags=0, extra=b"", name=b"", comment=b"", crc=None, isize=None, mtime=0, xfl=0, os_=3):
    """one RFC 1952 member around the raw DEFLATE stream of `text`; crc / isize override the trailer (damage)"""
    flg = flags | (4 if extra else 0) | (8 if name else 0) | (16 if comment else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<IBB", mtime, xfl, os_)
    if extra:
        h += struct.pack("<H", len(extra)) + extra
    if name:
        h += name + b"\0"
    if comment:
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    tr = struct.pack("<II", (zlib.crc32(text) if crc is None else crc) & 0xFFFFFFFF, (len(text) if isize is None else isize) & 0xFFFFFFFF)
    return h + bu.deflate_raw(text, level, strategy) + tr


@functools.lru_cache(maxsize=None)
def text_a():
    return bu.fastq_text(3000, 100, seed=3)


@functools.lru_cache(maxsize=None)
def text_c():
    """matches that reach far back across every cut: 20 000 random bytes repeated with a period of 30 000"""
    rng = random.Random(21)
    rep = bytes(rng.getrandbits(8) for _ in range(20000))
    out = []
    for i in range(14):
        out.append(rep + bytes(rng.getrandbits(8) for _ in range(10000)))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def valid_cases():
    """{name: (gzip bytes, text)} -- (a) to (f)"""
    a, out = text_a(), {}
    for level in (1, 6, 9):
        out[f"a_level{level}"] = (gz_member(a, level), a)
    for strat in ("fixed", "huffman", "rle"):
        out[f"b_{strat}"] = (gz_member(a, 6, strat), a)
    out["b_stored"] = (gz_member(a, 0), a)
    out["c_far_matches"] = (gz_member(text_c(), 6), text_c())
    # (d) three members: the first ends inside a chunk of 8 KiB and of 32 KiB, the second is padded (FEXTRA of the third) so that the third starts on a
    # multiple of 32 KiB, and the third is empty
    t1, t2 = a[:150000], a[150000:400000]
    m1, m2 = gz_member(t1, 6), gz_member(t2, 9)
    pad = (-(len(m1) + len(m2))) % 32768
    if pad < 4:
        pad += 32768
    m2 = gz_member(t2, 9, comment=b"c" * (pad - 1))                 # the comment and its zero byte: pad bytes more
    assert (len(m1) + len(m2)) % 32768 == 0 and len(m1) % 8192 != 0
    out["d_three_members"] = (m1 + m2 + gz_member(b""), t1 + t2)
    out["e_header_fields"] = (gz_member(a[:90000], 6, flags=2, extra=b"XY\x03\x00abc", name=b"reads.fastq", comment=b"made by a test", mtime=1700000000, xfl=2, os_=255), a[:90000])
    raw = bu.deflate_raw(a, 6)                                      # (f) stored blocks full of bit offsets at which a dynamic header parses, all of them false
    out["f_deflate_inside_stored"] = (gz_member(raw, 0), raw)
    for name, (blob, text) in out.items():
        assert gzip.decompress(blob) == text, name
    return out


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """{name: gzip bytes} -- (g): each must be refused"""
    a = text_a()
    good = gz_member(a, 6)
    out = {}
    b = bytearray(good)
    b[len(good) * 3 // 4] ^= 0x10                                   # one flipped bit in the DEFLATE data of a late chunk
    out["g_bit_flip"] = bytes(b)
    out["g_wrong_crc"] = gz_member(a, 6, crc=zlib.crc32(a) ^ 1)
    out["g_wrong_isize"] = gz_member(a, 6, isize=len(a) + 1)
    out["g_cut_in_block"] = good[:len(good) // 2]
    out["g_cut_in_trailer"] = good[:-3]
    out["g_garbage_behind"] = good + b"\x00\x01\x02\x03\x04"
    for name, blob in out.items():
        try:
            ok = gzip.decompress(blob) is not None
        except Exception:
            ok = False
        assert not ok, name
    return out
