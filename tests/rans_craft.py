"""An encoder that takes orders, for the three packed side files (README: "The packed quality file", "The packed id file", "The packed stream file"): plain
Python over integers, written from the README's format text and importing nothing from the library.  The table, the start state and the symbol or event
sequence of every strand are arguments, and every block is an object whose head fields, table rows, strand lengths and strand bytes the caller may change
before the bytes are made: what the library's encoders never write, valid or not.  The decoders written from the README (tests/readme_decoders.py) are its
independent check."""
import struct
import zlib

LOW = 1 << 23
TOT = 4096


# ------------------------------------------------------------------------------------------------ the coder
def encode(steps, start=LOW, lazy_first=False):
    """steps: (freq, cum) of every symbol of a strand in the order the decoder meets them -> the strand's bytes: the final state, most significant byte first,
    then the renormalisation bytes in the order the decoder reads them.  The symbols are walked last to first from `start`; a byte leaves while the state is at
    least freq << 19, which keeps the state after the step below 2^31.  lazy_first: the step of the strand's first symbol lets bytes leave only while the state is
    at least freq << 20, so its result -- the first state of the strand -- may be anything below 2^32; the decoder's first step undoes it without reading a byte"""
    x, tail = start, bytearray()
    for k in range(len(steps) - 1, -1, -1):
        f, c = steps[k]
        assert 1 <= f <= TOT and 0 <= c and c + f <= TOT, (f, c)
        limit = f << (20 if lazy_first and k == 0 else 19)
        while x >= limit:
            tail.append(x & 255)
            x >>= 8
        x = ((x // f) << 12) + x % f + c
    assert x < 1 << 32
    return x.to_bytes(4, "big") + bytes(reversed(tail))


def cums(freq):
    c, out = 0, []
    for f in freq:
        out.append(c)
        c += f
    return out


def spread(counts):
    """a row of counts -> frequencies that sum to 4096, by a rule that is not the library's: every count > 0 gets 1, the other 4096 - k are shared in proportion,
    rounded down, and what is left goes one each to the largest remainders, the highest symbol first on ties.  A row without a count stays all zero"""
    T, k = sum(counts), sum(1 for c in counts if c)
    if not T:
        return [0] * len(counts)
    rest = TOT - k
    f = [1 + c * rest // T if c else 0 for c in counts]
    order = sorted((y for y, c in enumerate(counts) if c), key=lambda y: (-(counts[y] * rest % T), -y))
    for y in order[:TOT - sum(f)]:
        f[y] += 1
    assert sum(f) == TOT
    return f


def _per_strand(v, s, default):
    return v.get(s, default) if isinstance(v, dict) else v


def _u32s(v):
    return struct.pack("<%dI" % len(v), *[x & 0xFFFFFFFF for x in v])


def _u16s(v):
    return struct.pack("<%dH" % len(v), *v)


class Block:
    """what the three blocks share: `u32 payload_bytes` (self.payload_bytes when set, else the payload's length) in front of the payload"""
    payload_bytes = None

    def bytes(self):
        p = self.payload()
        return struct.pack("<I", len(p) if self.payload_bytes is None else self.payload_bytes) + p


def _file(magic, fields, blocks):
    return magic + struct.pack("<IIQQ", *fields) + b"".join(b if isinstance(b, bytes) else b.bytes() for b in blocks)


# ------------------------------------------------------------------------------------------------ the packed quality file
class QualityBlock(Block):
    """m lines of L bytes.  alphabet: the byte values of the bitmap, ascending (default: those that occur); rows: (A + 1) rows of A frequencies to code with (default:
    norm over the counts of every (context, symbol) pair); start / lazy_first: per strand, {strand: value} or one value for all; stored: mode 0.
    Afterwards: mode, A, bitmap (an integer), rows, lens[256], strands[256], body (mode 0), payload_bytes"""

    def __init__(self, lines, L, alphabet=None, rows=None, norm=spread, start=LOW, lazy_first=False, stored=False):
        assert all(len(ln) == L for ln in lines)
        self.m, self.L = len(lines), L
        self.mode, self.body = (0, b"".join(lines)) if stored else (1, None)
        if stored:
            return
        syms = sorted(set(b"".join(lines))) if alphabet is None else list(alphabet)
        A = len(syms)
        self.A, self.bitmap = A, sum(1 << (v - 33) for v in syms)
        num = {v: y for y, v in enumerate(syms)}
        if rows is None:
            counts = [[0] * A for _ in range(A + 1)]
            for ln in lines:
                ctx = A
                for v in ln:
                    counts[ctx][num[v]] += 1
                    ctx = num[v]
            rows = [norm(r) for r in counts]
        self.rows = [list(r) for r in rows]
        cum = [cums(r) for r in rows]
        self.strands = []
        for s in range(256):
            steps = []
            for ln in lines[s::256]:
                ctx = A
                for v in ln:
                    y = num[v]
                    steps.append((rows[ctx][y], cum[ctx][y]))
                    ctx = y
            self.strands.append(encode(steps, _per_strand(start, s, LOW), _per_strand(lazy_first, s, False)) if steps else b"")
        self.lens = [len(x) for x in self.strands]

    def payload(self):
        if self.body is not None:
            return bytes([self.mode]) + self.body
        return bytes([self.mode, self.A]) + self.bitmap.to_bytes(12, "little") + b"".join(_u16s(r) for r in self.rows) + _u32s(self.lens) + b"".join(self.strands)


def quality_file(blocks, L, rb, n=None):
    n = sum(b.m for b in blocks) if n is None else n
    return _file(b"HARCQ1\0\0", (L, rb, n, 0), blocks)


# ------------------------------------------------------------------------------------------------ the packed stream file
def stream_row(freq, present=None):
    """a row in the file: 32 bytes of symbol bitmap and the u16 frequencies of the symbols named there (default: those with a frequency)"""
    present = [y for y in range(256) if freq[y]] if present is None else sorted(present)
    return sum(1 << y for y in present).to_bytes(32, "little") + _u16s([freq[y] for y in present])


class StreamBlock(Block):
    """m bytes of text in mode 0, 1 or 2.  rows: {row: 256 frequencies} to code with (mode 1: row 0 alone; default: norm over the counts; rows the text never uses may
    be given).  Afterwards: mode, text_bytes, crc, rows ({row: 256 frequencies, or bytes that go into the file as they are}), row_bitmap (None: the keys of rows),
    lens[256], strands[256], body (mode 0), payload_bytes"""

    def __init__(self, text, mode, rows=None, norm=spread, start=LOW, lazy_first=False):
        m = len(text)
        self.m, self.mode, self.text_bytes, self.crc, self.row_bitmap = m, mode, m, zlib.crc32(text), None
        self.body = text if mode == 0 else None
        if mode == 0:
            return
        q = (m + 255) // 256
        parts = [text[min(m, s * q):min(m, (s + 1) * q)] for s in range(256)]
        if rows is None:
            counts = {}
            for part in parts:
                ctx = 0
                for v in part:
                    counts.setdefault(ctx, [0] * 256)[v] += 1
                    ctx = v if mode == 2 else 0
            rows = {r: norm(c) for r, c in counts.items()}
        self.rows = {r: list(f) for r, f in rows.items()}
        cum = {r: cums(f) for r, f in rows.items()}
        self.strands = []
        for s, part in enumerate(parts):
            steps, ctx = [], 0
            for v in part:
                steps.append((rows[ctx][v], cum[ctx][v]))
                ctx = v if mode == 2 else 0
            self.strands.append(encode(steps, _per_strand(start, s, LOW), _per_strand(lazy_first, s, False)) if steps else b"")
        self.lens = [len(x) for x in self.strands]

    def payload(self):
        head = struct.pack("<BII", self.mode, self.text_bytes, self.crc)
        if self.body is not None:
            return head + self.body
        rows = b"".join(r if isinstance(r, bytes) else stream_row(r) for _, r in sorted(self.rows.items()))
        if self.mode != 1:
            rows = (sum(1 << r for r in self.rows) if self.row_bitmap is None else self.row_bitmap).to_bytes(32, "little") + rows
        return head + rows + _u32s(self.lens) + b"".join(self.strands)


def stream_file(blocks, B, n=None):
    n = sum(b.m for b in blocks) if n is None else n
    return _file(b"HARCS1\0\0", (B, 0, n, 0), blocks)


# ------------------------------------------------------------------------------------------------ the packed id file
MATCH, DELTA, NUM, STR, END = range(5)


def id_row_width(r):
    return 5 if r < 16 else 256 if r < 28 else 96


def id_events(ops):
    """the ops of one line -> its events (row, symbol), END included.  An op is (MATCH,), (DELTA, difference), (NUM, value) or (STR, bytes): whatever the case
    author orders, applicable or not"""
    ev, t = [], 0
    for op in ops:
        ev.append((min(t, 15), op[0]))
        if op[0] == DELTA:
            ev.append((16 + min(t, 7), op[1]))
        elif op[0] == NUM:
            ev += [(24 + k, op[1] >> 8 * k & 255) for k in range(4)]
        elif op[0] == STR:
            ctx = 0
            for v in op[1]:
                ev.append((28 + ctx, v - 31))
                ctx = v - 31
            ev.append((28 + ctx, 0))
        t += 1
    return ev + [(min(t, 15), END)]


class IdBlock(Block):
    """m lines.  ops: the ops of every line (id_events); text: the lines as the block declares them, newlines included -- the strand text bytes and block_text_bytes
    come from them, the decoder writes what the ops say.  rows: {row: frequencies} to code with (default: norm over the counts of the events).  stored: mode 0 with
    b"".join(text) as its bytes.  Afterwards: mode, text_bytes, stext[256], lens[256], rows, bitmap (None: the keys of rows), strands[256], body, payload_bytes"""

    def __init__(self, ops, text, rows=None, norm=spread, start=LOW, lazy_first=False, stored=False):
        m = len(text)
        self.m, self.text_bytes, self.bitmap = m, sum(len(t) for t in text), None
        self.mode, self.body = (0, b"".join(text)) if stored else (1, None)
        if stored:
            return
        assert len(ops) == m
        q = (m + 255) // 256
        cut = [(min(m, s * q), min(m, (s + 1) * q)) for s in range(256)]
        events = [[e for line in ops[a:b] for e in id_events(line)] for a, b in cut]
        self.stext = [sum(len(t) for t in text[a:b]) for a, b in cut]
        if rows is None:
            counts = {}
            for ev in events:
                for r, y in ev:
                    counts.setdefault(r, [0] * id_row_width(r))[y] += 1
            rows = {r: norm(c) for r, c in counts.items()}
        self.rows = {r: list(f) for r, f in rows.items()}
        cum = {r: cums(f) for r, f in rows.items()}
        self.strands = [encode([(rows[r][y], cum[r][y]) for r, y in ev], _per_strand(start, s, LOW), _per_strand(lazy_first, s, False)) if ev else b""
                        for s, ev in enumerate(events)]
        self.lens = [len(x) for x in self.strands]

    def payload(self):
        head = struct.pack("<BI", self.mode, self.text_bytes)
        if self.body is not None:
            return head + self.body
        bits = sum(1 << r for r in self.rows) if self.bitmap is None else self.bitmap
        return head + _u32s(self.stext) + _u32s(self.lens) + bits.to_bytes(16, "little") + b"".join(_u16s(f) for _, f in sorted(self.rows.items())) + b"".join(self.strands)


def id_file(blocks, rb, n=None, text_bytes=None):
    n = sum(b.m for b in blocks) if n is None else n
    text_bytes = sum(b.text_bytes for b in blocks) if text_bytes is None else text_bytes
    return _file(b"HARCI1\0\0", (rb, 0, n, text_bytes), blocks)


def block_offsets(f):
    """the byte of every block of a crafted file, by the u32 payload_bytes in front of each"""
    at, off = 32, []
    while at + 4 <= len(f):
        off.append(at)
        at += 4 + struct.unpack_from("<I", f, at)[0]
    return off
