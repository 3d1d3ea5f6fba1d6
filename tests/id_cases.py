"""Id texts for the packed id file (X.id.hi): three real-looking sets of 20 000 ids, and small cases that are each only as large as the block coder needs to go
wrong.  Shared by tests/test_idpack_host.py (no GPU) and tests/test_gpu_idpack.py."""
import functools
import random
import struct

TAIL = b" HWI-ST:lane-C:ABCACXX:tile-x:y-pos length=hundred/bases"     # 56 bytes without a digit: one string token, so that a line alone stays under the event bound


def ids(n, start=1000000, step=1):
    """@run<i><TAIL>: a string, a number of seven digits, a string -- 74 events for 68 bytes and their 2 when the line is the first of its strand"""
    return [b"@run%d%s" % (start + step * i, TAIL) for i in range(n)]


def text(lines):
    return b"".join(l + b"\n" for l in lines)


@functools.lru_cache(maxsize=None)
def illumina_ids():
    """the 20 000 ids of tests/bgzf_out_cases.illumina_text, in order"""
    from tests import bgzf_out_cases as oc
    return tuple(oc.illumina_text().split(b"\n")[0:-1:4])


@functools.lru_cache(maxsize=None)
def real_sets():
    """{name: text}"""
    il = list(illumina_ids())
    assert len(il) == 20000 and sum(len(x) + 1 for x in il) == 1428535
    sh = list(il)
    random.Random(5).shuffle(sh)                                   # what -c -q without -p leaves
    srr = [b"@SRR1234567.%d %d length=100" % (i, i) for i in range(1, 20001)]
    return {"illumina_in_order": text(il), "illumina_shuffled": text(sh), "srr": text(srr)}


# Sequences of lines that must sit next to each other in one strand.  small_cases() puts each at the second line of a strand of 12
NEIGHBOURS = {
    "values_at_the_limit": [b"@run999999998 x", b"@run999999999 x", b"@run1000000000 x", b"@run999999999 x", b"@run1000000001 x"],
    "leading_zeros": [b"@run007 x", b"@run008 x", b"@run8 x", b"@run0 x", b"@run00 x", b"@run0 x", b"@run1 x"],
    "differences": [b"@run5000 x", b"@run5000 x", b"@run5001 x", b"@run5256 x", b"@run5512 x", b"@run5511 x", b"@run0 x", b"@run255 x", b"@run511 x"],
    "fewer_and_more_tokens": [b"@run5 a1b2c3 x", b"@run5", b"@run5 a1b2c3d4e5 x", b"@run6 a1b2c3", b"", b"@run6 a1b2c3", b"9", b"9a"],
    "more_than_16_tokens": [b"@run5 " + b"1:" * 20, b"@run5 " + b"1:" * 18 + b"2:3:", b"@run5 " + b"1:" * 18 + b"9:3:7:7", b"@run5 " + b"2;" * 20],
    "digits_only": [b"123456", b"123457", b"1234570000", b"0", b"00", b"999999999", b"999999999"],
}


def small_cases():
    """{name: (text, lines_per_block)}; 0 = the default block"""
    rng = random.Random(31)
    c = {}
    for m in (1, 255, 256, 257, 513):                              # strands without lines, q = 1, 2, 3, a last strand that is short or empty
        c["m_%d" % m] = (text(ids(m)), 0)
    for n in (299, 300, 301, 901):                                 # block cuts, a last block of one line
        c["cut_%d_RB300" % n] = (text(ids(n, step=3)), 300)
    c["empty"] = (b"", 0)
    c["empty_lines"] = (text([b"" if i % 3 == 1 else l for i, l in enumerate(ids(898))] + [b"", b""]), 300)
    c["only_empty_lines"] = (b"\n" * 700, 300)
    c["digits_only_lines"] = (text([b"%d" % (1000000 + 7 * i) for i in range(3000)]), 0)
    base = ids(3000)                                               # q = 12
    k = 2
    for name in sorted(NEIGHBOURS):
        seq = NEIGHBOURS[name]
        base[12 * k + 1:12 * k + 1 + len(seq)] = seq
        k += 3
    c["neighbours"] = (text(base), 0)
    for name in sorted(NEIGHBOURS):                                # ... and each alone, in a block of its own size: q = 1, every line against an empty one
        c["alone_" + name] = (text(NEIGHBOURS[name]), 0)
    bad = ids(900)
    bad[450] = bad[450][:20] + b"\t" + bad[450][21:]
    bad[460] = bad[460][:9] + b"\x80" + bad[460][10:]
    c["tab_and_0x80_middle_block_stored"] = (text(bad), 300)
    c["random_bytes_stored"] = (text([bytes(rng.randrange(32, 127) for _ in range(60)) for _ in range(300)]), 0)
    c["random_letters_stored"] = (text([bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ_-+/=.:,;!?#$%&()*<>@[]^{|}~") for _ in range(60)) for _ in range(300)]), 0)
    c["1a1a_stored_by_the_event_bound"] = (text([b"1a" * 30] * 600), 0)
    # 39 common differences and 150 rare ones in one row of 256: more entries lifted to 1 than the largest frequency, 4096 / 39, can pay for
    v, vals = 1000, []
    for i in range(30000):
        v += 100 + i // 200 if i % 200 == 0 else rng.randrange(1, 40)
        vals.append(b"%d" % v)
    c["more_lifted_entries_than_the_largest_frequency"] = (text(vals), 0)
    long = ids(300)
    long[100] = b"@run1000100 " + b"abc" * 13329 + b"x"               # 40 000 bytes
    assert len(long[100]) == 40000
    c["one_id_of_40000_bytes"] = (text(long), 0)
    return c


# the modes of the blocks of every small case: what each case is there for
MODES = {
    "m_1": [0],                                                    # one line cannot pay for the head
    "m_255": [1], "m_256": [1], "m_257": [1], "m_513": [1],
    "cut_299_RB300": [1], "cut_300_RB300": [1], "cut_301_RB300": [1, 0], "cut_901_RB300": [1, 1, 1, 0],
    "empty": [],
    "empty_lines": [1, 1, 1], "only_empty_lines": [0, 0, 0],
    "digits_only_lines": [1],
    "neighbours": [1],
    "tab_and_0x80_middle_block_stored": [1, 0, 1],
    "random_bytes_stored": [0], "random_letters_stored": [0], "1a1a_stored_by_the_event_bound": [0],
    "one_id_of_40000_bytes": [1], "more_lifted_entries_than_the_largest_frequency": [1],
}
MODES.update({"alone_" + k: [0] for k in NEIGHBOURS})


def corruption_text():
    return text(ids(600))


def corrupted(packed, seed=13):
    """{name: bytes}: the damaged forms of a one-block mode-1 file `packed`.  Every name but wrong_magic must be refused naming block 0"""
    assert packed[36] == 1
    stext, slen, bitmap, tab = 41, 41 + 1024, 41 + 2048, 41 + 2048 + 16
    bits = int.from_bytes(packed[bitmap:bitmap + 16], "little")
    width = lambda r: 5 if r < 16 else 256 if r < 28 else 96
    strands = tab + 2 * sum(width(r) for r in range(124) if bits >> r & 1)
    rng = random.Random(seed)
    out = {}
    for k in range(60):
        b = bytearray(packed)
        bit = rng.randrange(8 * strands, 8 * len(packed))
        b[bit >> 3] ^= 1 << (bit & 7)
        out["flip_%02d" % k] = bytes(b)

    def poke(fmt, at, d):
        b = bytearray(packed)
        v = struct.unpack_from(fmt, b, at)[0]
        struct.pack_into(fmt, b, at, v + d)
        return bytes(b)

    def xor(at, v):
        b = bytearray(packed)
        b[at] ^= v
        return bytes(b)
    first = next(i for i in range((strands - tab) // 2) if struct.unpack_from("<H", packed, tab + 2 * i)[0] > 1)
    present = next(r for r in range(124) if bits >> r & 1)
    absent = next(r for r in range(124) if not bits >> r & 1)
    out["mode_2"] = xor(36, 3)
    out["payload_bytes_plus_1"] = poke("<I", 32, 1)
    out["payload_bytes_minus_1"] = poke("<I", 32, -1)
    out["block_text_bytes_plus_1"] = poke("<I", 37, 1)
    out["block_text_bytes_minus_1"] = poke("<I", 37, -1)
    out["strand_text_bytes_plus_1"] = poke("<I", stext + 4 * 7, 1)
    moved = bytearray(poke("<I", stext + 4 * 7, 1))                 # the sum stays, strand 7 ends a byte late
    struct.pack_into("<I", moved, stext + 4 * 8, struct.unpack_from("<I", moved, stext + 4 * 8)[0] - 1)
    out["strand_text_bytes_moved"] = bytes(moved)
    out["strand_length_plus_1"] = poke("<I", slen + 4 * 7, 1)
    out["strand_length_minus_1"] = poke("<I", slen + 4 * 7, -1)
    out["bitmap_bit_past_the_rows"] = xor(bitmap + 15, 0x80)
    out["bitmap_present_row_cleared"] = xor(bitmap + present // 8, 1 << present % 8)
    out["bitmap_absent_row_set"] = xor(bitmap + absent // 8, 1 << absent % 8)
    out["row_sum_plus_1"] = poke("<H", tab + 2 * first, 1)
    out["row_sum_minus_1"] = poke("<H", tab + 2 * first, -1)
    out["truncated_tail"] = packed[:-3]
    out["truncated_in_the_head"] = packed[:36 + 700]
    out["trailing_bytes"] = packed + b"\0\0"
    out["header_text_bytes_plus_1"] = poke("<Q", 24, 1)
    out["header_lines_plus_1"] = poke("<Q", 16, 1)
    out["wrong_magic"] = b"HARCI2" + packed[6:]
    return out
