"""A DEFLATE writer and a token reader in plain Python (RFC 1951), for streams that zlib's encoder never writes: any distance up to 32 768, code-length runs
that cross from the literal/length lengths into the distance lengths, full tables with 15-bit codes, single codes, empty blocks of every type.  The writer takes
tokens (an int is a literal, (length, distance) a match) and the code lengths of both trees as the caller states them; the reader lists what a stream holds so
that a test can state facts about it.  The reference for text is always zlib.  Test infrastructure only; nothing of the project is imported."""
import struct
import zlib

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LITLEN = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8      # 288 codes: 286 and 287 have codes and no meaning
FIXED_DIST = (5,) * 32                                             # 32 codes: 30 and 31 have codes and no meaning


# ---------------------------------------------------------------------------------------------------------------- writer
class BitWriter:
    """bits LSB first (RFC 1951 3.1.1); a Huffman code goes first bit first, so `code` writes it reversed"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, val, bits):
        self.acc |= (val & ((1 << bits) - 1)) << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, bits):
        r = 0
        for _ in range(bits):
            r = (r << 1) | (code & 1)
            code >>= 1
        self.put(r, bits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bits(self):
        return len(self.out) * 8 + self.n

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """{symbol: (code, bits)} of the canonical code with these lengths (RFC 1951 3.2.2); complete or not, as the caller made them"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def _balanced(c, depth):
    """lengths of c leaves that fill one node at `depth`"""
    k = c.bit_length() - 1
    return [depth + k] * ((2 << k) - c) + [depth + k + 1] * (2 * (c - (1 << k)))


def complete(n, chain=0):
    """the lengths (sorted) of a complete code of n symbols.  chain = 0: balanced.  chain = 2 .. 14: that many leaves form a chain that ends in two codes of
    15 bits (15, 15, 14, 13, ...: together one node at depth 16 - chain); the other leaves fill the siblings of that node's path from the root"""
    if chain == 0:
        assert n >= 2
        return sorted(_balanced(n, 0))
    d = 16 - chain
    assert 2 <= chain <= 14 and n - chain >= d, (n, chain)
    out = [15, 15] + list(range(14, 16 - chain, -1))
    rest = n - chain
    for depth in range(1, d + 1):                                  # the sibling at every depth of the path takes half of what is left, and at least one
        below = d - depth
        c = rest if depth == d else max(1, min(rest - below, (rest + 1) // 2))
        out += _balanced(c, depth)
        rest -= c
    assert len(out) == n and max(out) == 15 and sum(1 << (15 - l) for l in out) == 1 << 15, (n, chain)
    return sorted(out)


def length_symbol(length):
    """-> (symbol 257 .. 285, extra bits, their value).  258 is written as symbol 285"""
    s = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def symbols_of(tokens):
    """(literal/length symbols, distance symbols) that the tokens use; end-of-block included"""
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        else:
            ls.add(length_symbol(t[0])[0])
            ds.add(dist_symbol(t[1])[0])
    return ls, ds


def put_tokens(w, tokens, lit, dist, end=True):
    """lit / dist: canonical(...) of the block's trees"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
            continue
        s, eb, ev = length_symbol(t[0])
        w.code(*lit[s])
        w.put(ev, eb)
        s, eb, ev = dist_symbol(t[1])
        w.code(*dist[s])
        w.put(ev, eb)
    if end:
        w.code(*lit[256])


def stored_block(w, data, final=False, nlen=None):
    """nlen overrides the complement (damage)"""
    assert len(data) <= 65535
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    w.out += data


def fixed_block(w, tokens, final=False):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, tokens, canonical(FIXED_LITLEN), canonical(FIXED_DIST))


def run_length(lengths):
    """the code-length symbols of RFC 1951 3.2.7 for a list of lengths, greedily: [(symbol, extra value)].  The list is taken as one, so a run does not
    stop where the literal/length lengths end"""
    ops, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        r = j - i
        if v == 0:
            while r >= 11:
                k = min(r, 138); ops.append((18, k - 11)); r -= k
            if r >= 3:
                ops.append((17, r - 3)); r = 0
        else:
            ops.append((v, 0)); r -= 1
            while r >= 3:
                k = min(r, 6); ops.append((16, k - 3)); r -= k
        ops += [(v, 0)] * r
        i = j
    return ops


def dynamic_block(w, tokens, final, litlen_lengths, dist_lengths, ops=None, end=True):
    """HLIT = len(litlen_lengths) - 257 and HDIST = len(dist_lengths) - 1 as five bits each, whatever they are; the code-length code is complete over the
    symbols that the run-length coding of litlen_lengths + dist_lengths uses (ops overrides that coding: damage)"""
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(litlen_lengths) - 257, 5)
    w.put(len(dist_lengths) - 1, 5)
    if ops is None:
        ops = run_length(list(litlen_lengths) + list(dist_lengths))
    used = sorted({s for s, _ in ops})
    if len(used) == 1:                                             # one code of one bit would be incomplete: a second symbol takes the other half
        used = sorted(set(used) | {0 if used[0] else 1})
    cl = [0] * 19
    for s, l in zip(used, complete(len(used))):
        cl[s] = l
    hclen = max(max(k for k in range(19) if cl[CL_ORDER[k]]) + 1, 4)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl[CL_ORDER[k]], 3)
    cc = canonical(cl)
    for s, ev in ops:
        w.code(*cc[s])
        if s >= 16:
            w.put(ev, (2, 3, 7)[s - 16])
    put_tokens(w, tokens, canonical(litlen_lengths), canonical(dist_lengths), end)


def lengths_for(symbols, n, chain=0, rng=None):
    """n code lengths: a complete code (complete(len(symbols), chain)) over `symbols`, dealt out in an order that rng shuffles; 0 for every other symbol.  One
    symbol alone gets one bit (the incomplete code that RFC 1951 3.2.7 allows)"""
    symbols = sorted(symbols)
    out = [0] * n
    ls = [1] if len(symbols) == 1 else complete(len(symbols), chain)
    if rng:
        rng.shuffle(ls)
    for s, l in zip(symbols, ls):
        out[s] = l
    return out


def expand(tokens, text=b""):
    """the text of the tokens behind `text`"""
    out = bytearray(text)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= len(out), (t, len(out))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out[len(text):])


def gz(raw, text):
    """a bare RFC 1952 member around a raw DEFLATE stream whose text is `text`"""
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------- token reader
class _Bits:
    def __init__(self, raw, at=0):
        self.raw, self.pos, self.acc, self.n = raw + bytes(8), at, 0, 0

    def need(self, k):
        while self.n < k:
            self.acc |= self.raw[self.pos] << self.n
            self.pos += 1
            self.n += 8

    def take(self, k):
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def align(self):
        self.pos -= self.n // 8                                    # whole bytes that were taken in ahead
        self.acc, self.n = 0, 0

    def symbol(self, table, bits):
        self.need(bits)
        s, l = table[self.acc & ((1 << bits) - 1)]
        self.acc >>= l
        self.n -= l
        return s


def _table(lengths):
    """(lookup by the next `bits` bits, bits)"""
    bits = max(lengths) if max(lengths, default=0) else 1
    table = [(-1, 1)] * (1 << bits)
    for s, (code, l) in canonical(lengths).items():
        r = int(format(code, "0%db" % l)[::-1], 2)
        table[r::1 << l] = [(s, l)] * (1 << (bits - l))
    return table, bits


def tokens(raw, at=0):
    """the blocks of the raw DEFLATE stream at raw[at:], for streams that zlib accepts: ([{bit, type, final, hlit, hdist, maxbits, ncodes, cross, cross_at, tokens}], the
    byte behind the stream).  bit: where the block starts, counted from raw[at]; type: 0 stored (its tokens are its bytes), 1 fixed, 2 dynamic; maxbits and
    ncodes: the longest code and the number of codes of (the literal/length tree, the distance tree); cross: the repeat code (16, 17, 18) whose run crosses
    from the literal/length lengths into the distance lengths, or None, and cross_at: where that run starts, counted from the first distance length (0 or less)"""
    b, out = _Bits(raw, at), []
    while True:
        bit = (b.pos - at) * 8 - b.n
        final, btype = b.take(1), b.take(2)
        blk = {"bit": bit, "type": btype, "final": final, "hlit": None, "hdist": None, "maxbits": None, "ncodes": None, "cross": None, "cross_at": None, "tokens": []}
        if btype == 0:
            b.align()
            n = struct.unpack_from("<H", b.raw, b.pos)[0]
            blk["tokens"] = list(b.raw[b.pos + 4:b.pos + 4 + n])
            b.pos += 4 + n
        else:
            if btype == 1:
                ll, dl = list(FIXED_LITLEN), list(FIXED_DIST)
            else:
                assert btype == 2
                hlit, hdist, hclen = b.take(5), b.take(5), b.take(4)
                cl = [0] * 19
                for k in range(hclen + 4):
                    cl[CL_ORDER[k]] = b.take(3)
                ct, cb = _table(cl)
                lens = []
                while len(lens) < hlit + 257 + hdist + 1:
                    s, was = b.symbol(ct, cb), len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.take(2))
                    else:
                        lens += [0] * (3 + b.take(3) if s == 17 else 11 + b.take(7))
                    if was - (s == 16) < hlit + 257 < len(lens):   # a run that crosses from one tree's lengths into the other's; code 16 also crosses
                        blk["cross"], blk["cross_at"] = s, was - hlit - 257      # when it starts at the first distance length: it repeats the last literal/length length
                assert len(lens) == hlit + 257 + hdist + 1
                ll, dl = lens[:hlit + 257], lens[hlit + 257:]
                blk["hlit"], blk["hdist"] = hlit, hdist
            blk["maxbits"] = (max(ll), max(dl))
            blk["ncodes"] = (sum(1 for l in ll if l), sum(1 for l in dl if l))
            (lt, lb), (dt, db) = _table(ll), _table(dl)
            toks = blk["tokens"]
            while True:
                s = b.symbol(lt, lb)
                if s < 256:
                    toks.append(s)
                    continue
                if s == 256:
                    break
                s -= 257
                length = LEN_BASE[s] + b.take(LEN_EXTRA[s])
                d = b.symbol(dt, db)
                toks.append((length, DIST_BASE[d] + b.take(DIST_EXTRA[d])))
        out.append(blk)
        if final:
            return out, b.pos - b.n // 8


def gz_tokens(blob):
    """the blocks of every member of a gzip byte string (BGZF included): [[block, ...] per member]"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 3] == b"\x1f\x8b\x08", at
        flg, p = blob[at + 3], at + 10
        if flg & 4:
            p += 2 + struct.unpack_from("<H", blob, p)[0]
        for f in (8, 16):
            if flg & f:
                p = blob.index(b"\0", p) + 1
        if flg & 2:
            p += 2
        blocks, end = tokens(blob, p)
        out.append(blocks)
        at = end + 8
    return out


def max_distance(blocks):
    return max((t[1] for blk in blocks if blk["type"] for t in blk["tokens"] if not isinstance(t, int)), default=0)
