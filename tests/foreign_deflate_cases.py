"""DEFLATE streams in dialects that zlib's encoder never writes (tests/deflate_craft.py writes them), for tests/test_gunzip_host.py, tests/test_bgzf_host.py and
tests/test_gpu_gunzip_foreign.py: distances up to 32 768, full tables with 15-bit codes, code-length runs that cross from one tree into the other, single codes,
empty blocks of every type, stored blocks of 65 535 bytes.  Each is seeded and built once.  Every valid stream is accepted by zlib with the text of its tokens,
every refused one is refused by zlib, both asserted where the case is built.  Test infrastructure only."""
import functools
import random
import zlib

from tests import bgzf_util as bu
from tests import deflate_craft as dc

FAR = (32768, 32767, 32766, 32507, 32506, 24577, 16385)


def zlib_says(blob):
    """None when zlib inflates every member of the gzip bytes, else its message"""
    try:
        while blob:
            d = zlib.decompressobj(31)
            d.decompress(blob)
            if not d.eof:
                return "the stream ends early"
            blob = d.unused_data
    except zlib.error as e:
        return str(e)
    return None


def dyn(w, toks, final=False, chain=0, dchain=0, nlit=None, dist=None, rng=None):
    """a dynamic block whose trees hold exactly the symbols of its tokens: a complete code over them (a chain of `chain` leaves down to 15 bits), one bit for a
    symbol that is alone, HLIT and HDIST as low as the symbols allow (nlit: more literal/length lengths; dist: the distance lengths as given)"""
    ls, ds = dc.symbols_of(toks)
    litlen = dc.lengths_for(ls, max(nlit or 0, max(ls) + 1, 257), chain, rng)
    if dist is None:
        dist = dc.lengths_for(ds, max(ds) + 1, dchain, rng) if ds else [0]
    dc.dynamic_block(w, toks, final, litlen, dist)


def mixed(rng, have, n, p_match=0.3):
    """n tokens behind `have` bytes of text: random literals, and matches of every length symbol at every distance symbol that `have` allows"""
    out = []
    for _ in range(n):
        if have < 1 or rng.random() >= p_match:
            out.append(rng.getrandbits(8)); have += 1
            continue
        s = rng.randrange(29)
        length = dc.LEN_BASE[s] + rng.getrandbits(dc.LEN_EXTRA[s])
        if length > 258:
            length = 258
        d = rng.choice([k for k in range(30) if dc.DIST_BASE[k] <= have])
        dist = min(dc.DIST_BASE[d] + rng.getrandbits(dc.DIST_EXTRA[d]), have)
        out.append((length, dist)); have += length
    return out, have


def _far(D):
    rng = random.Random(D)
    w, toks, left, i = dc.BitWriter(), [], D + 3000, 0
    while left:
        k = left if left <= 900 else min(rng.randrange(200, 901), left - 200)
        lits = [rng.getrandbits(8) for _ in range(k)]
        nd = rng.randrange(2, 31)                                  # no distance is used: none has a code, or codes that nothing uses
        dist = ([0], [0] * nd, [0] * (nd - 2) + [1, 1], dc.complete(nd))[i % 4]
        dyn(w, lits, chain=(0, 5, 12)[i % 3], nlit=257 + rng.randrange(30), dist=dist, rng=rng)
        toks += lits; left -= k; i += 1
    for L in (3, 258, 4, 257, 130):                                # each in a block of its own: two literal/length codes and one distance code, of one bit each
        dyn(w, [(L, D)])
        toks.append((L, D))
    last = [(258, D), (258, 1), (258, D), (3, D)]
    dyn(w, last, final=True)
    return w.bytes(), toks + last


def _full_tables():
    rng = random.Random(286)
    w, toks, have = dc.BitWriter(), [], 0
    for cl, cd in ((5, 12), (12, 5), (2, 14), (14, 2)):
        t, have = mixed(rng, have, 300, 0.0)
        t2, have = mixed(rng, have, 400, 0.3)
        # every code has a length.  Blocks 0 and 2: the two 15-bit codes of the literal/length tree come last and those of the distance tree first, so a run of
        # code 16 starts in one tree and ends in the other.  Blocks 1 and 3: the last literal/length length is alone of its value and the first three distance
        # lengths have it, so code 16 is the first distance length's and repeats a length of the other tree
        a, b = dc.complete(286, cl), dc.complete(30, cd)
        rng.shuffle(a); rng.shuffle(b)
        x, na, nb = (15, 2, 2) if cl < cd else (max(v for v in a if b.count(v) >= 3), 1, 3)
        a = [x] * (a.count(x) - na) + [v for v in a if v != x] + [x] * na
        b = [x] * nb + [v for v in b if v != x] + [x] * (b.count(x) - nb)
        dc.dynamic_block(w, t + t2, False, a, b)
        toks += t + t2
    dyn(w, [0], final=True)
    return w.bytes(), toks + [0]


def _one_dist_and_empties(runs=300):
    w = dc.BitWriter()
    a = [65, 66, 67, (3, 3), (10, 3), 68, (4, 3)]                   # a single distance code (symbol 2, one bit)
    dyn(w, a)
    b = [ord(c) for c in "no distance code at all: the one distance length is zero\n"] * 3
    dyn(w, b)
    dc.dynamic_block(w, [], False, [0] * 256 + [1], [0])            # only end-of-block: one literal/length code of one bit
    dc.stored_block(w, b"")
    dc.fixed_block(w, [])
    c = [88] + [(258, 1)] * runs
    dyn(w, c, final=True)
    return w.bytes(), a + b + c


def _pigz_like():
    rng = random.Random(128)
    w, toks, have = dc.BitWriter(), [], 0
    for i in range(5):
        t, have = mixed(rng, have, 1500, 0.05)
        dyn(w, t, chain=(0, 5, 12)[i % 3], dchain=0, rng=rng)
        dc.stored_block(w, b"")
        dc.stored_block(w, b"")
        toks += t
    dc.fixed_block(w, [], final=True)
    return w.bytes(), toks


def _empty_walks():
    rng = random.Random(60)
    w = dc.BitWriter()
    a = [rng.getrandbits(8) for _ in range(1500)]
    dyn(w, a, chain=5, rng=rng)
    for _ in range(60):
        dc.stored_block(w, b"")
    b = [(100, 1500), (258, 700), 7, (3, 1859), (258, 1)]
    dyn(w, b)
    for _ in range(60):
        dc.stored_block(w, b"")
    c = [(258, 1800), (50, 1), 9, (258, 2400)]
    dc.fixed_block(w, c)
    d = [1, 2, 3, (3, 3)]
    dyn(w, d, final=True)
    return w.bytes(), a + b + c + d


def _stored_65535():
    rng = random.Random(65535)
    w = dc.BitWriter()
    s1, s2 = (bytes(rng.getrandbits(8) for _ in range(65535)) for _ in range(2))
    dc.stored_block(w, s1)
    a = [(258, 32768)] * 10
    dyn(w, a)
    dc.stored_block(w, s2)
    b = [(258, 32768), (3, 32768)]
    dc.fixed_block(w, b)
    dc.stored_block(w, b"", final=True)
    return w.bytes(), list(s1) + a + list(s2) + b


def _starts_behind_1024_chunks():
    """two stored blocks of 65 535 bytes, then dynamic blocks of more than 64 bytes each: in chunks of 64 bytes their starts lie in chunks 2048 and up, which
    the finder's 1024 waves reach only by their stride, and the chain lands on them"""
    rng = random.Random(1024)
    w = dc.BitWriter()
    s1, s2 = (bytes(rng.getrandbits(8) for _ in range(65535)) for _ in range(2))
    dc.stored_block(w, s1)
    dc.stored_block(w, s2)
    toks = []
    for i in range(7):
        t = [rng.getrandbits(8) for _ in range(100)] + [(258, 32768), (3 + i, 32768 - i)]
        dyn(w, t, final=i == 6, rng=rng)
        toks += t
    return w.bytes(), list(s1) + list(s2) + toks


def _fixed_only_far():
    rng = random.Random(1)
    w, toks = dc.BitWriter(), []
    for _ in range(7):
        t = [rng.getrandbits(8) for _ in range(5000)]
        dc.fixed_block(w, t)
        toks += t
    t = [(258, 32768), (3, 32767), 5, (258, 32768), (130, 1)]
    dc.fixed_block(w, t, final=True)
    return w.bytes(), toks + t


@functools.lru_cache(maxsize=None)
def raw_streams():
    """{name: (raw DEFLATE, tokens, text)}"""
    out = {f"far_{D}": _far(D) for D in FAR}
    out["full_tables"] = _full_tables()
    out["one_dist_and_empties"] = _one_dist_and_empties()
    out["pigz_like"] = _pigz_like()
    out["empty_walks"] = _empty_walks()
    out["stored_65535"] = _stored_65535()
    out["fixed_only_far"] = _fixed_only_far()
    out["starts_behind_1024_chunks"] = _starts_behind_1024_chunks()
    return {name: (raw, toks, dc.expand(toks)) for name, (raw, toks) in out.items()}


@functools.lru_cache(maxsize=None)
def valid_cases():
    """{name: (gzip bytes, text)}"""
    out = {name: (dc.gz(raw, text), text) for name, (raw, _, text) in raw_streams().items()}
    t1 = bu.fastq_text(100, 100, seed=41)
    raw, _, t2 = raw_streams()["far_32768"]
    out["two_members"] = (dc.gz(bu.deflate_raw(t1, 6), t1) + dc.gz(raw, t2), t1 + t2)
    for name, (blob, text) in out.items():
        got, at = b"", blob
        while at:                                                   # member by member: zlib.decompress stops behind the first
            d = zlib.decompressobj(31)
            got += d.decompress(at)
            assert d.eof, name
            at = d.unused_data
        assert got == text, name
        assert len(blob) <= 140000, (name, len(blob))
    return out


def _refused_blocks():
    """{name: (write the refused block into a writer, what zlib says)}; each is the only block of its member"""
    good_lit, good_dist = dc.lengths_for([65, 256], 257), [1]
    ops = dc.run_length(good_lit + good_dist)

    def hdr(nlit, ndist):
        return lambda w: dc.dynamic_block(w, [0], True, dc.complete(nlit), dc.complete(ndist))

    def fixed_raw(lsym, dsym=None):
        def f(w):
            w.put(1, 1); w.put(1, 2)
            lit, dist = dc.canonical(dc.FIXED_LITLEN), dc.canonical(dc.FIXED_DIST)
            w.code(*lit[65])
            w.code(*lit[lsym])
            if dsym is not None:
                w.code(*dist[dsym])
            w.code(*lit[256])
        return f
    out = {}
    for v in (30, 31):
        out[f"hlit_{v}"] = (hdr(257 + v, 30), "too many length or distance symbols")
        out[f"hdist_{v}"] = (hdr(286, 1 + v), "too many length or distance symbols")
    out["repeat_16_first"] = (lambda w: dc.dynamic_block(w, [65], True, good_lit, good_dist, ops=[(16, 0)] + ops), "invalid bit length repeat")
    out["run_overshoots"] = (lambda w: dc.dynamic_block(w, [65], True, good_lit, good_dist, ops=ops[:-1] + [(18, 127)]), "invalid bit length repeat")
    two = [0] * 257
    two[65] = two[256] = 2                                          # two codes of two bits: half of the code space is unused
    out["litlen_incomplete"] = (lambda w: dc.dynamic_block(w, [65], True, two, [1]), "invalid literal/lengths set")
    for s in (286, 287):
        out[f"fixed_length_{s}"] = (fixed_raw(s), "invalid literal/length code")
    for s in (30, 31):
        out[f"fixed_distance_{s}"] = (fixed_raw(257, s), "invalid distance code")
    out["stored_len_nlen"] = (lambda w: dc.stored_block(w, b"stored", True, nlen=(6 ^ 0xFFFF) ^ 0x0100), "invalid stored block lengths")
    return out


@functools.lru_cache(maxsize=None)
def refused_cases():
    """{name: (gzip bytes, lo, hi, what zlib says)}; [lo, hi]: the compressed bytes of the first block of the member that is refused"""
    out = {}
    for name, (write, says) in _refused_blocks().items():
        w = dc.BitWriter()
        write(w)
        out[name] = (dc.gz(w.bytes() + bytes(4), b""), 10, 10 + len(w.bytes()), says)
    for n in (10, 4999, 32767):                                    # a distance that reaches one byte before the member's start, the text in several dynamic blocks
        rng = random.Random(n)
        w, left, first = dc.BitWriter(), n, None
        while left:
            k = min(left, max(4, n // 7 + 1))
            left -= k
            lits = [rng.getrandbits(8) for _ in range(k)]
            dyn(w, lits + ([(3, n + 1)] if not left else []), final=not left, rng=rng)
            first = first or len(w.bytes())
        out[f"distance_before_start_{n}"] = (dc.gz(w.bytes(), b""), 10, 10 + first, "invalid distance too far back")
    # a second member whose first token reaches back into the first: the window restarts with every member
    rng = random.Random(2)
    t1 = bytes(rng.getrandbits(8) for _ in range(40000))
    m1 = dc.gz(bu.deflate_raw(t1, 6), t1)
    w = dc.BitWriter()
    dyn(w, [(3, 1), 65], final=True)
    out["second_member_reaches_back"] = (m1 + dc.gz(w.bytes(), b""), len(m1) + 10, len(m1) + 10 + len(w.bytes()), "invalid distance too far back")
    for name, (blob, lo, hi, says) in out.items():
        assert zlib_says(blob) is not None and says in zlib_says(blob), (name, zlib_says(blob))
    return out


@functools.lru_cache(maxsize=None)
def bgzf_members():
    """{name: (BGZF member, text)}: the crafted streams of 65 536 bytes of text or less, each as the CDATA of one member"""
    pick = {name: (raw, text) for name, (raw, _, text) in raw_streams().items() if len(text) <= 65536}
    raw, toks = _one_dist_and_empties(200)
    pick["one_dist_and_empties"] = (raw, dc.expand(toks))
    out = {}
    for name, (raw, text) in pick.items():
        assert len(text) <= 65536, name
        out[name] = (bu.member(text, cdata=raw), text)
        assert zlib.decompress(out[name][0], 31) == text, name
    return out


@functools.lru_cache(maxsize=None)
def bgzf_refused_members():
    """{name: BGZF member}: the refused blocks as the CDATA of one member whose trailer claims a byte of text"""
    out = {}
    for name, (write, _) in _refused_blocks().items():
        w = dc.BitWriter()
        write(w)
        out[name] = bu.member(b"A", cdata=w.bytes() + bytes(4))
        assert zlib_says(out[name]) is not None, name
    w = dc.BitWriter()
    dyn(w, [1, 2, 3, (3, 4), 65], final=True)
    out["distance_before_start_3"] = bu.member(b"A" * 7, cdata=w.bytes())
    assert "too far back" in zlib_says(out["distance_before_start_3"])
    return out
