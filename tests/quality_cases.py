"""Quality texts for the packed quality file (harc_amd/csrc/qv_block.h, qpack.hip), shared by the host test and the GPU test: three generators of realistic
lines, and for every part of the coder the smallest text at which it can go wrong.  A case is (text, L, reads_per_block); reads_per_block 0 = the default."""
import random

from tests import bgzf_out_cases as boc


def _clamp(x, lo, hi):
    return lo if x < lo else hi if x > hi else x


def markov(n, L, seed=1):
    """lines that start high and decay, some with a tail of quality 2"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        q = _clamp(int(rng.gauss(37, 3)), 2, 41)
        tail = rng.randrange(L // 2, L) if rng.random() < 0.15 and L > 1 else L
        ln = bytearray()
        for t in range(L):
            if rng.random() < 0.35:
                q = _clamp(q + int(rng.gauss(-0.3 - t / L, 3)), 2, 41)
            ln.append(33 + (2 if t >= tail else q))
        out.append(bytes(ln) + b"\n")
    return b"".join(out)


def iid(n, seed=11):
    """the quality lines of bgzf_out_cases.illumina_text: 33 + clamp(int(gauss(30, 6)), 2, 40), L = 100"""
    return b"".join(ln + b"\n" for ln in boc.illumina_text(n, seed).split(b"\n")[3::4])


def eight_bin(n, L, seed=3):
    """the eight levels of a binned sequencer; the level stays with probability 0.92, else a fresh draw weighted to the top"""
    rng = random.Random(seed)
    alphabet, w = b"#-7<AFJK", [1, 1, 2, 3, 5, 8, 13, 21]
    out = []
    for _ in range(n):
        ln, c = bytearray(), rng.choices(alphabet, w)[0]
        for _ in range(L):
            if rng.random() >= 0.92:
                c = rng.choices(alphabet, w)[0]
            ln.append(c)
        out.append(bytes(ln) + b"\n")
    return b"".join(out)


def _lines(rng, n, L, alphabet):
    return b"".join(bytes(rng.choice(alphabet) for _ in range(L)) + b"\n" for _ in range(n))


def skewed_rows(seed=5, L=50):
    """Fibonacci counts over 24 symbols plus each of the 94 symbols once, shuffled: rows in which many counts are lifted to 1"""
    a, b, syms = 1, 1, bytearray()
    for s in range(24):
        syms += bytes([40 + 3 * s]) * a
        a, b = b, a + b
    syms += bytes(range(33, 127))
    syms += bytes([40]) * (-len(syms) % L)
    random.Random(seed).shuffle(syms)
    return b"".join(bytes(syms[i:i + L]) + b"\n" for i in range(0, len(syms), L))


def small_cases():
    """{name: (text, L, reads_per_block)}"""
    rng = random.Random(29)
    c = {}
    for n in (1, 255, 256, 257, 511, 513):                         # strand boundaries; the single line is stored (the coded form is larger)
        c["strands_%d_L37" % n] = (markov(n, 37, seed=n), 37, 0)
    c["L1_5000"] = (_lines(rng, 5000, 1, b"FGH"), 1, 0)
    c["L100_700"] = (markov(700, 100, seed=2), 100, 0)
    c["L255_300"] = (markov(300, 255, seed=4), 255, 0)
    c["one_symbol"] = ((b"I" * 100 + b"\n") * 1000, 100, 0)        # all frequencies 4096, every strand 4 bytes
    dom = bytearray((b"K" * 100 + b"\n") * 3000)
    for i in rng.sample(range(3000 * 100), 5):
        dom[i // 100 * 101 + i % 100] = ord("#")
    c["dominant_symbol"] = (bytes(dom), 100, 0)                    # frequencies 1 and 4095: two renormalisation bytes in one step
    c["skewed_rows"] = (skewed_rows(), 50, 0)
    c["full_alphabet"] = (_lines(rng, 600, 255, bytes(range(33, 127))), 255, 0)
    bad = bytearray(markov(400, 37, seed=6))
    bad[200 * 38 + 5] = 0x80
    c["byte_0x80_stored"] = (bytes(bad), 37, 0)
    mid = bytearray(markov(900, 37, seed=7))
    mid[450 * 38 + 9] = 0x80
    c["middle_block_stored"] = (bytes(mid), 37, 300)
    c["empty"] = (b"", 37, 0)
    for n in (299, 300, 301, 600, 901):                            # block cuts
        c["cut_%d_RB300" % n] = (markov(n, 50, seed=100 + n), 50, 300)
    return c


def corruption_text():
    return markov(600, 100, seed=9)


def corrupted(packed, seed=13):
    """{name: bytes}: the damaged forms of a one-block mode-1 file `packed` (tests/test_qpack_host.py, 3)"""
    import struct
    assert packed[36] == 1
    A = packed[37]
    tab = 36 + 14
    lens = tab + 2 * (A + 1) * A
    strands = lens + 1024
    rng = random.Random(seed)
    out = {}
    for k in range(60):
        b = bytearray(packed)
        bit = rng.randrange(8 * strands, 8 * len(packed))
        b[bit >> 3] ^= 1 << (bit & 7)
        out["flip_%02d" % k] = bytes(b)

    def poke16(at, d):
        b = bytearray(packed)
        v = struct.unpack_from("<H", b, at)[0]
        struct.pack_into("<H", b, at, v + d)
        return bytes(b)

    def poke32(at, d):
        b = bytearray(packed)
        v = struct.unpack_from("<I", b, at)[0]
        struct.pack_into("<I", b, at, v + d)
        return bytes(b)
    first = next(i for i in range((A + 1) * A) if struct.unpack_from("<H", packed, tab + 2 * i)[0] > 1)
    out["row_sum_plus_1"] = poke16(tab + 2 * first, 1)
    out["row_sum_minus_1"] = poke16(tab + 2 * first, -1)
    out["strand_length_plus_1"] = poke32(lens + 4 * 7, 1)
    out["strand_length_minus_1"] = poke32(lens + 4 * 7, -1)
    for d in (1, -1):
        b = bytearray(packed)
        b[37] = A + d
        out["A_%+d" % d] = bytes(b)
    b = bytearray(packed)
    b[36] = 2
    out["mode_2"] = bytes(b)
    out["truncated_tail"] = packed[:-3]
    out["wrong_magic"] = b"HARCQ2" + packed[6:]
    return out
