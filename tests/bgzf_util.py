"""BGZF writer in plain Python (SAM/BAM specification 4.1): raw DEFLATE per member, the BC subfield, CRC-32, ISIZE and the EOF marker,
with knobs for the member size, zlib level and strategy, and extra subfields placed before BC.  Test infrastructure only."""
import random
import struct
import zlib

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}


def deflate_raw(data, level=6, strategy="default"):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, STRATEGIES[strategy])
    return co.compress(data) + co.flush()


def member(data, level=6, strategy="default", extra_before=b"", cdata=None, isize=None, crc=None, bsize_delta=0):
    """one BGZF member holding `data`; cdata / isize / crc / bsize_delta override what is written (corrupt members)"""
    cd = deflate_raw(data, level, strategy) if cdata is None else cdata
    xlen = len(extra_before) + 6
    bsize = 12 + xlen + len(cd) + 8 - 1 + bsize_delta
    if not 0 <= bsize <= 0xFFFF:
        raise ValueError(f"a member of {bsize + 1} bytes does not fit BSIZE")
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra_before + b"BC" + struct.pack("<HH", 2, bsize)
    tr = struct.pack("<II", (zlib.crc32(data) if crc is None else crc) & 0xFFFFFFFF, (len(data) if isize is None else isize) & 0xFFFFFFFF)
    return hdr + cd + tr


def bgzf(data, member_text=65280, level=6, strategy="default", extra_before=b"", eof=True):
    """data as BGZF: members of member_text bytes of text each, then the EOF marker (an empty member) that bgzip appends"""
    out = [member(data[i:i + member_text], level, strategy, extra_before) for i in range(0, len(data), member_text)]
    if eof:
        out.append(EOF_MARKER)
    return b"".join(out)


def members(blob):
    """[(offset, size)] of the members of a BGZF byte string, by the BSIZE chain"""
    out, at = [], 0
    while at < len(blob):
        xlen = struct.unpack_from("<H", blob, at + 10)[0]
        k, bsize = 0, None
        while k + 4 <= xlen:
            si, slen = blob[at + 12 + k:at + 14 + k], struct.unpack_from("<H", blob, at + 14 + k)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", blob, at + 16 + k)[0]
            k += 4 + slen
        out.append((at, bsize + 1))
        at += bsize + 1
    return out


def fastq_text(n, L=100, seed=1, id_len=None, crlf=False, n_rate=0.002):
    """n FASTQ records of L bases with varied ids and seeded, non-constant quality values"""
    rng = random.Random(seed)
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n):
        rid = b"@r%d.%d length=%d" % (seed, i, L) if id_len is None else b"@" + bytes(rng.choice(b"ABCDEFGHIJ") for _ in range(id_len))
        seq = bytes(rng.choice(b"ACGT") if rng.random() > n_rate else ord("N") for _ in range(L))
        q = bytes(33 + min(40, max(2, int(rng.gauss(30, 6)))) for _ in range(L))
        out.append(rid + nl + seq + nl + b"+" + nl + q + nl)
    return b"".join(out)
