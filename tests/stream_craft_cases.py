"""Packed stream files that the library's encoder never writes, built to order by tests/rans_craft.py from the README's format text: valid ones with their text,
and damaged ones with the block and the SV_E_* code that the README's rule gives -- written down here by hand, never computed by the decoder under test.
Shared by tests/test_craft_host.py (the sanitizer build and the host twin) and tests/test_gpu_craft.py (the kernel)."""
import random
import zlib

from tests import rans_craft as rc

MODE, SIZE, BITMAP, ROW, LENGTHS, SHORT, TRUNC, CONTEXT, END, CRC = range(1, 11)
CODES = set(range(1, 11))                                          # the enum of sv_block.h
HEX = b"0123456789abcdef"


def _bytes(m, alphabet, seed, weights=None):
    return bytes(random.Random(seed).choices(alphabet, weights, k=m))


def _starved(counts):
    """the most frequent symbol of the row gets 1; the lowest other symbol that occurs gets what is left after a 1 for every occurring symbol"""
    top = max(range(256), key=lambda y: counts[y])
    f = [1 if c else 0 for c in counts]
    other = next((y for y in range(256) if y != top and counts[y]), top)
    f[other] += 4096 - sum(f)
    return f


def _row(pairs):
    f = [0] * 256
    for y, v in pairs.items():
        f[y] = v
    return f


def valid():
    """{name: (file, text)}"""
    c = {}

    def one(name, text, mode, **kw):
        b = rc.StreamBlock(text, mode, **kw)
        c[name] = (rc.stream_file([b], len(text)), text)
        return b
    for mode in (1, 2):
        one("another_rule_mode_%d_m1063" % mode, _bytes(1063, HEX, 1 + mode), mode)
        # strands of 2, 2, ..., 2, 1, 0, ... bytes: the CRC terms of the strands differ
        one("another_rule_mode_%d_m257" % mode, _bytes(257, HEX, 3 + mode), mode)
        # coded although stored is smaller
        one("coded_where_stored_is_smaller_mode_%d_m1" % mode, b"\x00", mode)
        one("coded_where_stored_is_smaller_mode_%d_m255" % mode, _bytes(255, b"ab", 5 + mode), mode)
    one("most_frequent_symbol_f1_mode_1_m256", _bytes(256, b"abc", 8, [1, 2, 30]), 1, norm=_starved)
    one("most_frequent_symbol_f1_mode_2_m1063", _bytes(1063, b"abc", 9, [1, 2, 30]), 2, norm=_starved)
    # b is one byte in forty and has 1 of 4096: twelve bits, two renormalisation bytes in a step
    one("f4095_beside_f1_mode_1_m1063", _bytes(1063, b"ab", 10, [40, 1]), 1, rows={0: _row({97: 4095, 98: 1})})
    # byte values 0, 128 and 255 are absent from a used row, 1, 127, 129 and 254 present
    one("absent_symbols_at_start_middle_end_mode_1_m1063", _bytes(1063, b"\x01\x7f\x81\xfe", 11), 1)
    one("all_256_symbols_mode_1_m1063", bytes(range(256)) * 4 + bytes(39), 1, rows={0: [16] * 256})
    one("all_256_symbols_mode_2_m257", b"".join(bytes([0, y]) for y in range(128, 256)) + b"\x00", 2, rows={0: [16] * 256})
    # mode 2: rows 1 and 255 are present and valid, no byte is coded in them
    text = _bytes(1063, b"abc", 12)
    b = rc.StreamBlock(text, 2)
    rows = dict(b.rows)
    rows[1], rows[255] = [16] * 256, _row({0: 4095, 255: 1})
    one("mode_2_with_rows_that_are_never_used_m1063", text, 2, rows=rows)
    # mode 2 although mode 1 is smaller: nothing depends on the byte in front, the table is four rows instead of one
    text = _bytes(1063, b"abc", 13)
    b1, b2 = rc.StreamBlock(text, 1), one("mode_2_where_mode_1_is_smaller_m1063", text, 2)
    assert len(b1.payload()) < len(b2.payload())
    # the first state: the only byte of a strand has 16 of 4096, and the encoder lets no byte leave in front of it: 2^31 and the symbol's cumulative
    for mode in (1, 2):
        b = one("first_state_2_31_mode_%d_m256" % mode, _bytes(256, b"ab", 14), mode, rows={0: _row({97: 16, 98: 4080})}, lazy_first={s: True for s in range(0, 256, 2)})
        assert any(int.from_bytes(s[:4], "big") >= 1 << 31 for s in b.strands)
    # three blocks through the header's B: 257, 257 and 1 bytes in modes 1, 0 and 2
    text = _bytes(515, HEX, 15)
    blocks = [rc.StreamBlock(text[:257], 1), rc.StreamBlock(text[257:514], 0), rc.StreamBlock(text[514:], 2)]
    c["three_blocks_modes_1_0_2_n515"] = (rc.stream_file(blocks, 257), text)
    return c


def refusals():
    """{name: (file, (block, code))}"""
    c = {}

    def one(name, code, change, mode=1, m=1063, seed=20, **kw):
        b = rc.StreamBlock(_bytes(m, HEX, seed), mode, **kw)
        r = change(b)
        c["%s_mode_%d" % (name, mode)] = (rc.stream_file([b if r is None else r], m, n=m), (0, code))

    def setter(**kw):
        def change(b):
            for k, v in kw.items():
                setattr(b, k, v)
        return change

    def raw(cut=None, add=b""):
        """the payload cut to `cut` bytes or with bytes behind it, under a payload_bytes that says so"""
        def change(b):
            p = b.payload()[:cut] + add
            return len(p).to_bytes(4, "little") + p
        return change

    def row(r, y, d):
        def change(b):
            b.rows[r][y] += d
        return change

    def raw_row(r, data):
        def change(b):
            b.rows[r] = data(b.rows[r])
        return change

    def drop_row(r):
        def change(b):
            del b.rows[r]
        return change

    def strand(s, data=None, length=None):
        """data(old bytes) -> the new bytes of strand s; its length field follows unless `length` gives one"""
        def change(b):
            if data is not None:
                b.strands[s] = data(b.strands[s])
            b.lens[s] = len(b.strands[s]) if length is None else length(b.lens[s])
        return change

    def both(*changes):
        def change(b):
            for ch in changes:
                ch(b)
        return change

    def flip_crc(b):
        b.crc ^= 1 << 17
    spare, low_state = (lambda d: d + b"\0"), (lambda d: b"\x00\x7f\xff\xff" + d[4:])

    def cut_last(d):
        assert len(d) > 4                                          # a renormalisation byte goes, not one of the state
        return d[:-1]
    # ---- one violation each
    one("mode_3", MODE, setter(mode=3))
    one("mode_255", MODE, setter(mode=255))
    one("stored_payload_plus_1", SIZE, raw(add=b"\0"), mode=0)
    one("stored_payload_minus_1", SIZE, raw(cut=-1), mode=0)
    one("payload_ends_in_the_first_bitmap", SIZE, raw(cut=40))
    one("payload_ends_in_the_frequencies", SIZE, raw(cut=9 + 32 + 31))
    one("payload_ends_in_the_strand_sizes", SIZE, raw(cut=9 + 64 + 1023))
    one("payload_ends_in_a_rows_bitmap", SIZE, raw(cut=9 + 32 + 64 + 31), mode=2)
    one("symbol_bitmap_empty", BITMAP, raw_row(0, lambda f: bytes(32)))
    one("row_bitmap_empty", BITMAP, setter(row_bitmap=0), mode=2)
    one("symbol_bitmap_of_a_row_empty", BITMAP, raw_row(ord("7"), lambda f: bytes(32)), mode=2)
    for mode in (1, 2):
        one("row_sum_4095", ROW, row(0, ord("3"), -1), mode=mode)
        one("row_sum_4097", ROW, row(0, ord("e"), 1), mode=mode)
        one("present_symbol_without_a_frequency", ROW, raw_row(0, lambda f: rc.stream_row(f, [y for y in range(256) if f[y]] + [200])), mode=mode)
        one("length_sum_plus_1", LENGTHS, strand(7, length=lambda n: n + 1), mode=mode)
        one("length_sum_minus_1", LENGTHS, strand(7, length=lambda n: n - 1), mode=mode)
        one("payload_bytes_plus_1", LENGTHS, raw(add=b"\0"), mode=mode)
        one("payload_bytes_minus_1", LENGTHS, raw(cut=-1), mode=mode)
        one("strand_with_text_of_3_bytes", SHORT, strand(9, data=lambda d: d[:3]), mode=mode)
        one("strand_without_text_of_4_bytes", SHORT, strand(255, data=lambda d: rc.LOW.to_bytes(4, "big")), mode=mode, m=255)
        one("last_byte_removed", TRUNC, strand(3, data=cut_last), mode=mode)
        one("start_state_2_23_plus_1", END, lambda b: None, mode=mode, start={5: rc.LOW + 1})
        one("spare_byte_behind_a_strand", END, strand(6, data=spare), mode=mode)
        one("first_state_below_2_23", END, strand(2, data=low_state), mode=mode)
        one("one_crc_bit_wrong", CRC, flip_crc, mode=mode)
        one("another_text_under_the_right_crc", CRC, setter(crc=zlib.crc32(_bytes(1063, HEX, 21))), mode=mode)
    one("length_above_the_payload", LENGTHS, strand(255, length=lambda n: 0xFFFFFFF0))
    one("strand_without_text_of_1_byte", SHORT, strand(200, data=lambda d: b"\0"), m=257)
    one("one_crc_bit_wrong", CRC, flip_crc, mode=0)
    one("used_row_absent", CONTEXT, drop_row(ord("a")), mode=2)
    one("row_0_absent", CONTEXT, drop_row(0), mode=2)
    # ---- two violations: the smallest code
    for mode in (1, 2):
        one("bad_row_and_short_strand", ROW, both(row(0, ord("0"), 1), strand(9, data=lambda d: d[:3])), mode=mode)
        one("strand_0_truncated_strand_1_wrong_end", TRUNC, strand(0, data=cut_last), mode=mode, start={1: rc.LOW + 1})
        one("strand_0_wrong_end_strand_1_truncated", TRUNC, strand(1, data=cut_last), mode=mode, start={0: rc.LOW + 1})
        one("short_strand_and_wrong_length_sum", LENGTHS, strand(9, length=lambda n: 3), mode=mode)
        one("wrong_end_and_wrong_crc", END, both(strand(6, data=spare), flip_crc), mode=mode)
    one("used_row_absent_and_spare_byte", CONTEXT, both(strand(0, data=spare), drop_row(ord("a"))), mode=2)
    # ---- three blocks: the lowest damaged block, and there the smallest code
    def three(name, want, *changes):
        text = _bytes(771, HEX, 30)
        blocks = [rc.StreamBlock(text[a:a + 257], mode) for a, mode in ((0, 1), (257, 2), (514, 1))]
        for b, ch in zip(blocks, changes):
            if ch:
                ch(b)
        c[name] = (rc.stream_file(blocks, 257), want)
    three("blocks_1_and_2_damaged", (1, END), None, strand(4, data=spare), setter(mode=3))
    three("block_2_damaged", (2, ROW), None, None, row(0, ord("0"), -1))
    three("block_1_twice_and_block_2", (1, ROW), None, both(flip_crc, row(0, ord("1"), 1)), flip_crc)
    return c


def check_edges():
    """the condition on the valid cases: the decoder written from the README meets a slot at the low and at the high edge of a symbol's range and a step that
    reads two renormalisation bytes, and reads every case back"""
    from tests import readme_decoders as rd
    seen = dict.fromkeys(rd.SEEN, 0)
    rd.SEEN.update(seen)
    for name, (f, text) in sorted(valid().items()):
        assert rd.stream_decode(f)[0] == text, name
    seen.update(rd.SEEN)
    assert all(seen.values()), seen
    return seen
