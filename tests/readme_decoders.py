"""Decoders of the three packed side files in plain Python, written from the README's format text ("The packed quality file", "The packed id file", "The packed
stream file") and asserting the constraints it states.  They are the independent check of the library's host encoders (tests/test_{qpack,idpack,spack}_host.py)
and of the crafted files of tests/rans_craft.py.  SEEN counts what the coder steps met: a slot at the low and at the high edge of a symbol's range (for symbols
with a frequency of at least 2) and steps that read two renormalisation bytes."""
import re
import struct
import zlib

QUALITY_MAGIC = b"HARCQ1\0\0"
ID_MAGIC = b"HARCI1\0\0"
STREAM_MAGIC = b"HARCS1\0\0"
SEEN = {"slot_low": 0, "slot_high": 0, "two_bytes": 0}


def _see(slot, cum, freq, nbytes):
    if freq >= 2:
        SEEN["slot_low"] += slot == cum
        SEEN["slot_high"] += slot == cum + freq - 1
    SEEN["two_bytes"] += nbytes == 2


def quality_decode(f):
    """-> (text, modes).  Asserts the constraints the format text states: the table's, and every strand's end"""
    assert f[:8] == QUALITY_MAGIC
    L, RB, n, zero = struct.unpack_from("<IIQQ", f, 8)
    assert zero == 0
    at, out, modes = 32, [], []
    for b0 in range(0, n, RB) if n else []:
        m = min(n, b0 + RB) - b0
        size, = struct.unpack_from("<I", f, at)
        p = f[at + 4:at + 4 + size]
        assert len(p) == size
        at += 4 + size
        modes.append(p[0])
        if p[0] == 0:
            assert size == 1 + m * L
            out += [p[1 + i * L:1 + (i + 1) * L] + b"\n" for i in range(m)]
            continue
        assert p[0] == 1
        A = p[1]
        bits = int.from_bytes(p[2:14], "little")
        syms = [33 + k for k in range(96) if bits >> k & 1]
        assert len(syms) == A and 1 <= A <= 94 and syms[-1] <= 126
        freq = [struct.unpack_from("<%dH" % A, p, 14 + 2 * A * r) for r in range(A + 1)]
        cum = []
        for row in freq:
            assert sum(row) in (0, 4096)
            c = [0]
            for v in row:
                c.append(c[-1] + v)
            cum.append(c)
        lens = struct.unpack_from("<256I", p, 14 + 2 * A * (A + 1))
        pos = 14 + 2 * A * (A + 1) + 1024
        assert pos + sum(lens) == size
        lines = [None] * m
        for s in range(256):
            data, pos = p[pos:pos + lens[s]], pos + lens[s]
            if s >= m:
                assert not data
                continue
            x, k = int.from_bytes(data[:4], "big"), 4
            for i in range(s, m, 256):
                ctx, ln = A, bytearray()
                for _ in range(L):
                    slot = x & 4095
                    y = next(y for y in range(A) if cum[ctx][y] <= slot < cum[ctx][y] + freq[ctx][y])
                    assert freq[ctx][y] >= 1                       # an occurring pair
                    x, k0 = freq[ctx][y] * (x >> 12) + slot - cum[ctx][y], k
                    while x < 1 << 23:
                        x, k = x << 8 | data[k], k + 1
                    _see(slot, cum[ctx][y], freq[ctx][y], k - k0)
                    ln.append(syms[y]); ctx = y
                lines[i] = bytes(ln) + b"\n"
            assert x == 1 << 23 and k == len(data)                 # the integrity check of the format
        out += lines
    assert at == len(f)
    return b"".join(out), modes


# ------------------------------------------------------------------------------------------------ ids
def _width(r):
    return 5 if r < 16 else 256 if r < 28 else 96


class _Rans:
    def __init__(self, data):
        assert len(data) >= 4
        self.d, self.x, self.k = data, int.from_bytes(data[:4], "big"), 4
        assert self.x >= 1 << 23

    def get(self, row):
        assert row is not None                                     # a symbol from an absent row
        freq, cum, lut = row
        slot = self.x & 4095
        y = lut[slot]
        assert freq[y] >= 1
        self.x, k0 = freq[y] * (self.x >> 12) + slot - cum[y], self.k
        while self.x < 1 << 23:
            self.x, self.k = self.x << 8 | self.d[self.k], self.k + 1
        _see(slot, cum[y], freq[y], self.k - k0)
        return y


def id_decode(f):
    """-> (text, modes).  Asserts the constraints the format text states"""
    assert f[:8] == ID_MAGIC
    RB, zero, n, tbytes = struct.unpack_from("<IIQQ", f, 8)
    assert zero == 0
    if n == 0:
        assert RB == 0 and tbytes == 0 and len(f) == 32
    at, out, modes = 32, [], []
    for b0 in range(0, n, RB) if n else []:
        m = min(n, b0 + RB) - b0
        size, = struct.unpack_from("<I", f, at)
        p = f[at + 4:at + 4 + size]
        assert len(p) == size
        at += 4 + size
        mode, T = p[0], struct.unpack_from("<I", p, 1)[0]
        modes.append(mode)
        if mode == 0:
            assert size == 5 + T and p.count(b"\n", 5) == m and p.endswith(b"\n")
            out.append(p[5:])
            continue
        assert mode == 1
        stext = struct.unpack_from("<256I", p, 5)
        slen = struct.unpack_from("<256I", p, 5 + 1024)
        bits = int.from_bytes(p[5 + 2048:5 + 2048 + 16], "little")
        assert bits >> 124 == 0
        pos, rows = 5 + 2048 + 16, []
        for r in range(124):
            if not bits >> r & 1:
                rows.append(None)
                continue
            freq = struct.unpack_from("<%dH" % _width(r), p, pos)
            pos += 2 * _width(r)
            assert sum(freq) == 4096
            cum, lut = [], []
            for y, v in enumerate(freq):
                cum.append(len(lut))
                lut += [y] * v
            rows.append((freq, cum, lut))
        assert sum(stext) == T and pos + sum(slen) == size
        q = -(-m // 256)
        for s in range(256):
            nl = min(m, (s + 1) * q) - min(m, s * q)
            data, pos = p[pos:pos + slen[s]], pos + slen[s]
            if nl == 0:
                assert not data and stext[s] == 0
                continue
            dec, prev, strand = _Rans(data), b"", []
            for _ in range(nl):
                ptok, cur, t = re.findall(rb"[0-9]+|[^0-9]+", prev), bytearray(), 0
                while True:
                    op = dec.get(rows[min(t, 15)])
                    if op == 4:
                        break
                    pt = ptok[t] if t < len(ptok) else None
                    if op == 0:
                        assert pt is not None
                        cur += pt
                    elif op == 1:
                        assert pt is not None and re.fullmatch(rb"0|[1-9][0-9]{0,8}", pt)
                        d = dec.get(rows[16 + min(t, 7)])
                        assert 1 <= d <= 255 and int(pt) + d <= 999999999
                        cur += b"%d" % (int(pt) + d)
                    elif op == 2:
                        v = sum(dec.get(rows[24 + k]) << 8 * k for k in range(4))
                        assert v <= 999999999
                        cur += b"%d" % v
                    else:
                        ctx = 0
                        while True:
                            y = dec.get(rows[28 + ctx])
                            if y == 0:
                                break
                            cur.append(y + 31)
                            ctx = y
                        assert ctx
                    t += 1
                strand.append(bytes(cur) + b"\n")
                prev = bytes(cur)
            strand = b"".join(strand)
            assert len(strand) == stext[s]
            assert dec.x == 1 << 23 and dec.k == len(data)         # the integrity check of the format
            out.append(strand)
    assert at == len(f)
    text = b"".join(out)
    assert len(text) == tbytes
    return text, modes


# ------------------------------------------------------------------------------------------------ streams
def _row(p, at):
    """the row at p[at:]: 32 bytes of bitmap, the u16 frequencies of its symbols -> (freq[256], cum[256], the bytes it takes)"""
    bits = int.from_bytes(p[at:at + 32], "little")
    syms = [y for y in range(256) if bits >> y & 1]
    assert syms
    f = struct.unpack_from("<%dH" % len(syms), p, at + 32)
    assert all(v >= 1 for v in f) and sum(f) == 4096
    freq, cum, c = [0] * 256, [0] * 256, 0
    for y in range(256):
        cum[y] = c
        if bits >> y & 1:
            freq[y] = f[syms.index(y)]
            c += freq[y]
    return freq, cum, 32 + 2 * len(syms)


def stream_decode(f):
    """-> (text, modes).  Asserts the constraints the format text states"""
    assert f[:8] == STREAM_MAGIC
    B, zero, n, zero2 = struct.unpack_from("<IIQQ", f, 8)
    assert zero == 0 and zero2 == 0
    if n == 0:
        assert B == 0 and len(f) == 32
        return b"", []
    assert 1 <= B <= 1 << 30
    at, out, modes = 32, [], []
    for b0 in range(0, n, B):
        m = min(n, b0 + B) - b0
        size, = struct.unpack_from("<I", f, at)
        p = f[at + 4:at + 4 + size]
        assert len(p) == size
        at += 4 + size
        mode, tb, crc = struct.unpack_from("<BII", p, 0)
        assert tb == m and mode in (0, 1, 2)
        modes.append(mode)
        if mode == 0:
            assert size == 9 + m
            text = p[9:]
        else:
            rows, pos = {}, 9
            if mode == 1:
                fr, cu, k = _row(p, pos)
                rows, pos = {r: (fr, cu) for r in range(256)}, pos + k
            else:
                present = int.from_bytes(p[9:41], "little")
                pos = 41
                for r in range(256):
                    if present >> r & 1:
                        fr, cu, k = _row(p, pos)
                        rows[r], pos = (fr, cu), pos + k
            lens = struct.unpack_from("<256I", p, pos)
            pos += 1024
            assert pos + sum(lens) == size
            q = (m + 255) // 256
            text = bytearray()
            for s in range(256):
                data, pos = p[pos:pos + lens[s]], pos + lens[s]
                ns = min(m, (s + 1) * q) - min(m, s * q)
                if ns == 0:
                    assert not data
                    continue
                assert len(data) >= 4
                x, k, ctx = int.from_bytes(data[:4], "big"), 4, 0
                for _ in range(ns):
                    freq, cum = rows[ctx]                          # an absent row: a KeyError
                    slot = x & 4095
                    y = next(y for y in range(256) if freq[y] and cum[y] <= slot < cum[y] + freq[y])
                    x, k0 = freq[y] * (x >> 12) + slot - cum[y], k
                    while x < 1 << 23:
                        x, k = x << 8 | data[k], k + 1
                    _see(slot, cum[y], freq[y], k - k0)
                    text.append(y)
                    ctx = y if mode == 2 else 0
                assert x == 1 << 23 and k == len(data)             # the end of a strand
            text = bytes(text)
        assert len(text) == m and zlib.crc32(text) == crc
        out.append(text)
    assert at == len(f)
    return b"".join(out), modes
