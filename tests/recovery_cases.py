"""The recovery record restated in plain Python from the README's text ("The recovery record (X.hr)"): GF(2^8) over 0x11D by its own log/exp tables and bytewise
products, the digest D, the geometry of blocks, spans and groups, the record made from [(name, bytes)], read back and repaired -- no code shared with
harc_amd/csrc/gf_block.h -- and the cases the host twin and the kernels are held to."""
import random
import struct

MAGIC = b"HARCR1\0\0"
M64 = (1 << 64) - 1

# ------------------------------------------------------------------------------------------------ the field
EXP, LOG = [0] * 512, [0] * 256
_x = 1
for _k in range(255):
    EXP[_k], LOG[_x] = _x, _k
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
for _k in range(255, 512):
    EXP[_k] = EXP[_k - 255]


def mul(a, b):
    return 0 if a == 0 or b == 0 else EXP[LOG[a] + LOG[b]]


def inv(a):
    assert a != 0
    return EXP[255 - LOG[a]]


def cauchy(i, j):
    return inv(i ^ (128 + j))


def mul_bytes(c, data):
    if c == 0:
        return bytes(len(data))
    lc = LOG[c]
    return bytes(EXP[lc + LOG[v]] if v else 0 for v in data)


def xor_bytes(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def combine(sources, coef):
    """out[q] = XOR_s coef[q][s] * sources[s]"""
    out = []
    for row in coef:
        acc = bytes(len(sources[0]))
        for c, s in zip(row, sources):
            acc = xor_bytes(acc, mul_bytes(c, s))
        out.append(acc)
    return out


def invert(A):
    """the inverse of a square matrix over the field, by elimination"""
    e = len(A)
    M = [list(r) + [int(r_ == c) for c in range(e)] for r_, r in enumerate(A)]
    for col in range(e):
        piv = next(r for r in range(col, e) if M[r][col])
        M[col], M[piv] = M[piv], M[col]
        d = inv(M[col][col])
        M[col] = [mul(v, d) for v in M[col]]
        for r in range(e):
            if r != col and M[r][col]:
                f = M[r][col]
                M[r] = [v ^ mul(f, w) for v, w in zip(M[r], M[col])]
    return [r[e:] for r in M]


# ------------------------------------------------------------------------------------------------ the digest
def mix64(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    return x ^ x >> 33


def digest(data, first=0):
    """D: the sum over the bytes of mix64(((o + 1) << 8) | byte), o counted from `first`"""
    return sum(mix64(((first + o + 1) << 8) | b) for o, b in enumerate(data)) & M64


# ------------------------------------------------------------------------------------------------ the geometry
def groups_of_span(s, K, PCT):
    """-> G, [(k, m)] for the groups of a span of s blocks; block t is member t // G of group t % G"""
    G = -(-s // K)
    out = []
    for g in range(G):
        k = len(range(g, s, G))
        out.append((k, min(128, max(1, -(-k * PCT // 100)))))
    return G, out


def spans_of(nb, S):
    return [(a, min(nb, a + S) - a) for a in range(0, nb, S)]      # (first block, blocks)


def blocks_of(data, B):
    return [data[a:a + B] for a in range(0, len(data), B)]


def pad(block, B):
    return block + bytes(B - len(block))


# ------------------------------------------------------------------------------------------------ the record
def make_record(files, pct, B=65536, S=8192, K=128):
    """files: [(name, bytes)] -> the bytes of X.hr"""
    entries, digests, rblocks = b"", b"", b""
    for name, data in files:
        blocks = blocks_of(data, B)
        rec = []
        for t0, s in spans_of(len(blocks), S):
            G, groups = groups_of_span(s, K, pct)
            for g, (k, m) in enumerate(groups):
                members = [pad(blocks[t0 + j * G + g], B) for j in range(k)]
                rec += combine(members, [[cauchy(i, j) for j in range(k)] for i in range(m)])
        nm = name.encode()
        entries += struct.pack("<H", len(nm)) + nm + struct.pack("<QQQQ", len(data), digest(data), len(blocks), len(rec))
        digests += b"".join(struct.pack("<Q", digest(b)) for b in blocks) + b"".join(struct.pack("<Q", digest(b)) for b in rec)
        rblocks += b"".join(rec)
    hb = 48 + len(entries) + len(digests)
    head = MAGIC + struct.pack("<IIIIII", B, S, K, pct, len(files), 0) + struct.pack("<QQ", hb, 0) + entries + digests
    head = head[:40] + struct.pack("<Q", digest(head)) + head[48:]
    return head + rblocks + head + struct.pack("<Q", hb)


class Refused(Exception):
    pass


def _parse_head(h, size):
    if len(h) < 48 or h[:8] != MAGIC:
        raise Refused("magic")
    B, S, K, pct, nf, zero, hb, d = struct.unpack_from("<IIIIIIQQ", h, 8)
    if hb != len(h) or digest(h[:40] + bytes(8) + h[48:]) != d:
        raise Refused("digest")
    if not (16 <= B <= 1 << 24 and B % 16 == 0 and S >= 1 and 1 <= K <= 128 and 1 <= pct <= 100 and zero == 0):
        raise Refused("geometry")
    at, files = 48, []
    for _ in range(nf):
        if at + 2 > hb:
            raise Refused("entries")
        nl, = struct.unpack_from("<H", h, at)
        if at + 2 + nl + 32 > hb:
            raise Refused("entries")
        name = h[at + 2:at + 2 + nl].decode(errors="surrogateescape")
        n, D, nb, rb = struct.unpack_from("<QQQQ", h, at + 2 + nl)
        at += 2 + nl + 32
        if name in ("", ".", "..") or "/" in name or "\0" in name or name in [f["name"] for f in files]:
            raise Refused("name")
        if nb != -(-n // B) or nb > hb // 8 or rb > hb // 8:
            raise Refused("counts")
        if rb != sum(m for _, s in spans_of(nb, S) for _, m in groups_of_span(s, K, pct)[1]):
            raise Refused("counts")
        files.append(dict(name=name, n=n, D=D, nb=nb, rb=rb))
    if hb - at != 8 * sum(f["nb"] + f["rb"] for f in files):
        raise Refused("digests")
    R = sum(f["rb"] for f in files)
    if 2 * hb + R * B + 8 != size:
        raise Refused("size")
    for f in files:
        f["dd"] = list(struct.unpack_from("<%dQ" % f["nb"], h, at))
        at += 8 * f["nb"]
        f["rd"] = list(struct.unpack_from("<%dQ" % f["rb"], h, at))
        at += 8 * f["rb"]
    return dict(B=B, S=S, K=K, PCT=pct, hb=hb, files=files, R=R)


def read_head(rec):
    """-> (head, which copy): the first copy whose own digest holds; Refused when neither does"""
    size = len(rec)
    if size < 2 * 48 + 8:
        raise Refused("short")
    try:
        hb, = struct.unpack_from("<Q", rec, 32)
        if rec[:8] != MAGIC or hb < 48 or hb > (size - 8) // 2:
            raise Refused("first")
        return _parse_head(rec[:hb], size), 1
    except Refused:
        pass
    hb, = struct.unpack_from("<Q", rec, size - 8)
    if hb < 48 or hb > (size - 8) // 2:
        raise Refused("neither copy of the head holds")
    try:
        return _parse_head(rec[size - 8 - hb:size - 8], size), 2
    except Refused:
        raise Refused("neither copy of the head holds")


def repair(rec, rname, files, write=True):
    """rec: the bytes of X.hr, rname its base name; files: {name: bytes, or None / absent when the file is missing} -> (status, lines, {name: bytes after}).
    Raises Refused for what the whole run is refused for (no head, a longer file)"""
    H, which = read_head(rec)
    B, S, K, pct = H["B"], H["S"], H["K"], H["PCT"]
    for f in H["files"]:
        data = files.get(f["name"])
        if data is not None and len(data) > f["n"]:
            raise Refused("%s holds %d bytes, %s records %d" % (f["name"], len(data), rname, f["n"]))
    lines, after, all_ok, roff, rdamaged, rbad = [], dict(files), True, H["hb"], 0, {}
    for f in H["files"]:
        rb = [digest(rec[roff + r * B:roff + (r + 1) * B]) != f["rd"][r] for r in range(f["rb"])]
        rbad[f["name"]], rdamaged, roff = rb, rdamaged + sum(rb), roff + f["rb"] * B
    if which == 2:
        lines.append("[recovery] %s: the first copy of the head is damaged, the second holds" % rname)
    if rdamaged:
        lines.append("[recovery] %s: %d of %d recovery blocks damaged" % (rname, rdamaged, H["R"]))
    roff = H["hb"]
    for f in H["files"]:
        name, n, nb = f["name"], f["n"], f["nb"]
        data = files.get(name)
        missing = data is None
        data = b"" if missing else data
        present = nb if len(data) == n else len(data) // B         # whole blocks that are there; a cut block is lost
        blocks = blocks_of(data[:n if present == nb else present * B], B)
        bad = [t >= present or digest(blocks[t]) != f["dd"][t] for t in range(nb)]
        base, my_roff = 0, roff
        roff += f["rb"] * B
        if not any(bad) and not missing:
            lines.append("[recovery] %s ok" % name)
            continue
        fixes, solvable = [], True
        for sp, (t0, s) in enumerate(spans_of(nb, S)):
            G, groups = groups_of_span(s, K, pct)
            for g, (k, m) in enumerate(groups):
                lost = [j for j in range(k) if bad[t0 + j * G + g]]
                intact = [i for i in range(m) if not rbad[name][base + i]]
                if lost and len(lost) > len(intact):
                    lines.append("[recovery] %s NOT recoverable: span %d group %d has lost %d of %d blocks and holds %d recovery blocks" % (name, sp, g, len(lost), k, len(intact)))
                    solvable = False
                    break
                if lost:
                    fixes.append((t0, G, g, k, base, lost, intact[:len(lost)]))
                base += m
            if not solvable:
                break
        if not solvable:
            all_ok = False
            continue
        if not write:
            all_ok = False
            lines.append("[recovery] %s damaged: %d of %d blocks, recoverable" % (name, sum(bad), nb))
            continue
        new = blocks + [b""] * (nb - len(blocks))
        for t0, G, g, k, base, lost, recs in fixes:
            Ainv = invert([[cauchy(i, j) for j in lost] for i in recs])
            keep = [j for j in range(k) if j not in lost]
            sources = [pad(new[t0 + j * G + g], B) for j in keep] + [rec[my_roff + (base + i) * B:my_roff + (base + i + 1) * B] for i in recs]
            coef = []
            for q in range(len(lost)):
                row = []
                for j in keep:
                    v = 0
                    for r, i in enumerate(recs):
                        v ^= mul(Ainv[q][r], cauchy(i, j))
                    row.append(v)
                coef.append(row + Ainv[q])
            for q, blk in enumerate(combine(sources, coef)):
                t = t0 + lost[q] * G + g
                blk = blk[:min(B, n - t * B)]
                assert digest(blk) == f["dd"][t]
                new[t] = blk
        whole = b"".join(new)
        assert len(whole) == n and digest(whole) == f["D"]
        after[name] = whole
        lines.append("[recovery] %s repaired: %d of %d blocks" % (name, sum(bad), nb))
    status = 0 if all_ok and (write or (which == 1 and not rdamaged)) else 1
    return status, lines, after


# ------------------------------------------------------------------------------------------------ the cases
def _bytes(seed, n):
    return bytes(random.Random(seed).getrandbits(8) for _ in range(n))


def cases():
    """-> [dict(name, B, S, K, PCT, files=[(name, bytes)])]: every size at which the geometry takes another shape"""
    out = []

    def add(name, B, S, K, PCT, sizes):
        out.append(dict(name=name, B=B, S=S, K=K, PCT=PCT, files=[("f%d.bin" % i, _bytes("%s/%d" % (name, i), n)) for i, n in enumerate(sizes)]))
    add("sizes16", 16, 8192, 128, 10, [0, 1, 15, 16, 17])           # n in 0, 1, B - 1, B, B + 1; k = 1, m = 1; one lane
    add("b48", 48, 8192, 4, 50, [48 * 5 + 7])                       # three lanes; two groups of three, m = 2
    add("b1040", 1040, 8192, 128, 34, [1040 * 3 + 1])               # not a whole wave's 1 KiB; k = 4, m = 2
    add("kK", 16, 8192, 8, 25, [16 * 8])                            # k = K
    add("kK1", 16, 8192, 8, 25, [16 * 9])                           # k = K + 1: the second group appears
    add("m128", 16, 8192, 128, 100, [2048])                         # m = 128 at K = 128, PCT = 100
    add("spans3", 16, 4, 2, 50, [16 * 9 - 3])                       # three spans, the last of one block
    add("three", 16, 8192, 4, 50, [100, 0, 77])                     # three files, the middle one empty
    return out
