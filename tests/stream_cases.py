"""Byte strings for the packed stream file (harc_amd/csrc/sv_block.h, spack.hip), shared by the host test and the GPU test: for every part of the coder the
smallest text at which it can go wrong.  A case is (text, block_bytes); block_bytes 0 = the default 2^22.  A block of at most 1062 bytes is always stored (the
1024 bytes of strand sizes and the smallest head are more than its text), so the lengths around the strand count and around a block size of 1000 check the
stored path and the cut into blocks, and the sources come in texts long enough for a coded block to win."""
import random
import struct

from tests import gen

B1 = 1000


def skewed(n, seed=3, symbols=100):
    """i.i.d. over `symbols` byte values with weights 1 / (rank + 1)"""
    rng = random.Random(seed)
    vals = rng.sample(range(256), symbols)
    return bytes(rng.choices(vals, [1.0 / (k + 1) for k in range(symbols)], k=n))


def markov(n, seed=5, symbols=16):
    """first order: every byte is followed by its favourite successor with probability 0.85, else by any of the symbols"""
    rng = random.Random(seed)
    vals = rng.sample(range(1, 256), symbols)
    fav = {v: rng.choice(vals) for v in vals}
    out, c = bytearray(), vals[0]
    for _ in range(n):
        c = fav[c] if rng.random() < 0.85 else rng.choice(vals)
        out.append(c)
    return bytes(out)


def two_symbols(n, seed=7):
    rng = random.Random(seed)
    return bytes(rng.choices(b"ab", [9, 1], k=n))


def uniform(n, seed=9):
    rng = random.Random(seed)
    return bytes(rng.randrange(256) for _ in range(n))


def lifted_row(pairs=60000, seed=11):
    """the byte 0xFF in front of every other byte: its row holds 42 common symbols and 170 rare ones (three times each), more entries lifted to a frequency of 1
    than the largest frequency, about 4096 / 42, can pay for -- the case of id_cases.more_lifted_entries_than_the_largest_frequency in a row of 256"""
    rng = random.Random(seed)
    common, rare = list(range(1, 43)), list(range(60, 230))
    syms = rare * 3 + [rng.choice(common) for _ in range(pairs - 3 * len(rare))]
    rng.shuffle(syms)
    return b"".join(bytes([0xFF, s]) for s in syms)


def lifted_row_takes_the_excess_branch(text):
    """the normalisation rule on the row of 0xFF in plain Python: the floors lifted to 1 sum to more than 4096 plus the largest frequency"""
    c = [0] * 256
    for i in range(1, len(text)):
        if text[i - 1] == 0xFF and i % ((len(text) + 255) // 256) != 0:
            c[text[i]] += 1
    T = sum(c)
    f = [max(1, v * 4096 // T) for v in c if v]
    return sum(f) > 4096 + max(f)


def cycle(n):
    """abcabc...: under order 1 every byte follows from the one in front -- except the first of a strand, whose context is 0 whatever stands in front of it"""
    return (b"abc" * (n // 3 + 1))[:n]


def small_cases():
    """{name: (text, block_bytes)}"""
    c = {}
    for n in (0, 1, 255, 256, 257):                                # fewer bytes than strands, a byte per strand, uneven strands with empty ones at the end
        c["len_%d" % n] = (skewed(n, seed=n), 0)
    for n in (B1 - 1, B1, B1 + 1, 3 * B1 + 5):
        c["cut_%d_B%d" % (n, B1)] = (skewed(n, seed=n), B1)
    c["repeated_byte"] = (b"A" * 4100, 0)                          # q = 17: 241 strands of 17, one of 3, 14 empty; every frequency 4096, every strand 4 bytes
    c["two_symbols"] = (two_symbols(30000), 0)
    c["uniform_stored"] = (uniform(20000), 0)
    c["skewed"] = (skewed(60000), 0)
    c["markov"] = (markov(60000), 0)
    c["markov_3B5_B12000"] = (markov(36005, seed=6), 12000)        # three coded blocks and one of five bytes
    c["acgtn_lines"] = (gen.reads_text(13, 300, 100, 5000, err=0.02, n_frac=0.3), 0)
    c["lifted_row"] = (lifted_row(), 0)
    c["context_0_rule"] = (cycle(30000), 0)
    c["mixed_blocks_B20000"] = (cycle(20000) + uniform(20000, seed=2) + skewed(20000, seed=4), 20000)      # mode 2, stored, mode 1
    assert lifted_row_takes_the_excess_branch(c["lifted_row"][0])
    assert 0 not in c["context_0_rule"][0] and 0 not in c["markov"][0]
    return c


# the modes of the blocks of every case: what each case is there for
MODES = {
    "len_0": [], "len_1": [0], "len_255": [0], "len_256": [0], "len_257": [0],
    "cut_999_B1000": [0], "cut_1000_B1000": [0], "cut_1001_B1000": [0, 0], "cut_3005_B1000": [0, 0, 0, 0],
    "repeated_byte": [1], "two_symbols": [1], "uniform_stored": [0], "skewed": [1], "markov": [2], "markov_3B5_B12000": [2, 2, 2, 0],
    "lifted_row": [2], "context_0_rule": [2], "mixed_blocks_B20000": [2, 0, 1],
}


def blocks_of(packed):
    """[(offset, mode, text bytes)] of the blocks of a packed stream file, by its prefixes"""
    out, at = [], 32
    while at < len(packed):
        size, mode, tb = struct.unpack_from("<IBI", packed, at)
        out.append((at, mode, tb))
        at += 4 + size
    assert at == len(packed)
    return out


def check_modes(pack):
    """the host twin `pack(text, block_bytes)` codes every case in the modes it is there for -- and so at least one block of the set in each of the three"""
    seen = set()
    for name, (text, B) in sorted(small_cases().items()):
        modes = [m for _, m, _ in blocks_of(pack(text, B))]
        if name in MODES:
            assert modes == MODES[name], (name, modes)
        seen.update(modes)
    assert seen == {0, 1, 2}, seen


def corruption_texts():
    """{mode: text of one block}"""
    return {0: uniform(5000, seed=21), 1: skewed(40000, seed=22), 2: markov(40000, seed=23)}


def flips(packed, n=60, seed=13, lo=36):
    """n seeded single-bit flips behind the payload_bytes prefix of the one block of `packed`"""
    rng = random.Random(seed)
    out = {}
    for k in range(n):
        b = bytearray(packed)
        at = rng.randrange(lo, len(b))
        b[at] ^= 1 << rng.randrange(8)
        out["flip_%02d" % k] = bytes(b)
    return out


def header_violations(packed):
    """{name: bytes}: truncations and every violation of the file header and the block prefix, on a one-block file"""
    size, = struct.unpack_from("<I", packed, 32)
    v = {
        "wrong_magic": b"HARCQ1\0\0" + packed[8:],
        "reserved_12": packed[:12] + b"\1\0\0\0" + packed[16:],
        "reserved_24": packed[:24] + b"\1" + packed[25:],
        "block_size_0": packed[:8] + struct.pack("<I", 0) + packed[12:],
        "block_size_above_2_30": packed[:8] + struct.pack("<I", (1 << 30) + 1) + packed[12:],
        "text_bytes_plus_1": packed[:16] + struct.pack("<Q", struct.unpack_from("<Q", packed, 16)[0] + 1) + packed[24:],
        "no_text_but_blocks": packed[:8] + bytes(24) + packed[32:],
        "trunc_header": packed[:31],
        "trunc_prefix": packed[:40],
        "trunc_tail": packed[:-1],
        "trunc_half": packed[:32 + size // 2],
        "bytes_behind": packed + b"\0",
        "payload_bytes_plus_1": packed[:32] + struct.pack("<I", size + 1) + packed[36:],
        "payload_bytes_minus_1": packed[:32] + struct.pack("<I", size - 1) + packed[36:],
        "payload_bytes_8": packed[:32] + struct.pack("<I", 8) + packed[36:],
        "mode_3": packed[:36] + b"\3" + packed[37:],
        "block_text_bytes_minus_1": packed[:37] + struct.pack("<I", struct.unpack_from("<I", packed, 37)[0] - 1) + packed[41:],
    }
    return v


# what names block 0 at byte 32: everything behind a header that parses and can hold its blocks
NAMES_BLOCK_0 = ("trunc_tail", "trunc_half", "payload_bytes_plus_1", "payload_bytes_minus_1", "payload_bytes_8", "mode_3", "block_text_bytes_minus_1")
