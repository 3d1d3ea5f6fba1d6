"""Packed id files that the library's encoder never writes, built to order by tests/rans_craft.py from the README's format text: valid ones with their text, and
damaged ones with the block and the ID_E_* code that the README's rule gives -- written down here by hand, never computed by the decoder under test.  Shared by
tests/test_craft_host.py (the sanitizer build and the host twin) and tests/test_gpu_craft.py (the kernel).

A block is strands of filler lines (`@r.<i> x`, then MATCH DELTA MATCH against it) with the lines under test put into named strands as (ops, line) pairs: the
ops are what the strand codes, the line is what the block declares and what a valid case decodes to."""
from tests import rans_craft as rc
from tests.rans_craft import MATCH, DELTA, NUM, STR

MODE, SIZE, BITMAP, ROW, LENGTHS, SHORT, TRUNC, CONTEXT, END, PREV, VALUE, TEXT, EMPTY = range(1, 14)
CODES = set(range(1, 14))                                          # the enum of id_block.h


def _filler(s, k):
    i = 1000 * s + 7
    if k == 0:
        return [(STR, b"@r."), (NUM, i), (STR, b" x")], b"@r.%d x\n" % i
    return [(MATCH,), (DELTA, k), (MATCH,)], b"@r.%d x\n" % (i + k)


def _block(m, special=None, **kw):
    """m lines; special: {strand: [(ops, line), ...]} in place of the strand's filler lines, as many as the strand holds"""
    q = (m + 255) // 256
    ops, text = [], []
    for s in range(256):
        nl = min(m, (s + 1) * q) - min(m, s * q)
        lines = (special or {}).get(s, [_filler(s, k) for k in range(nl)])
        assert len(lines) == nl, (s, nl)
        ops += [o for o, _ in lines]
        text += [t for _, t in lines]
    return rc.IdBlock(ops, text, **kw), b"".join(text)


def _starved(counts):
    """the most frequent symbol of the row gets 1, and the lowest other symbol of the row -- whether it occurs or not -- what is left after a 1 for every other
    occurring symbol"""
    top = max(range(len(counts)), key=lambda y: counts[y])
    f = [1 if c else 0 for c in counts]
    other = next(y for y in range(len(counts)) if y != top)
    f[other] += 4096 - sum(f)
    return f


A12 = ([(STR, b"a"), (NUM, 12)], b"a12\n")
TWENTY = ([op for k in range(1, 11) for op in ((STR, b"a"), (NUM, k))], b"a1a2a3a4a5a6a7a8a9a10\n")
TWENTY_NEXT = ([(MATCH,), (DELTA, 1)] * 10, b"a2a3a4a5a6a7a8a9a10a11\n")
VALID_PAIRS = {
    "num_where_match_applies": [A12, ([(MATCH,), (NUM, 12)], b"a12\n")],
    "num_where_delta_applies": [A12, ([(MATCH,), (NUM, 13)], b"a13\n")],
    "str_for_a_numeric_token": [([(STR, b"123")], b"123\n"), ([(STR, b"124")], b"124\n")],
    "str_for_007": [([(STR, b"007")], b"007\n"), ([(MATCH,)], b"007\n")],
    "a_token_as_two_literals_and_match_of_the_rejoined_token": [([(STR, b"ab"), (STR, b"cd")], b"abcd\n"), ([(MATCH,)], b"abcd\n")],
    "delta_255": [([(NUM, 5)], b"5\n"), ([(DELTA, 255)], b"260\n")],
    "delta_onto_999999999": [([(NUM, 999999744)], b"999999744\n"), ([(DELTA, 255)], b"999999999\n")],
    "num_999999999": [([(NUM, 999999999)], b"999999999\n"), ([(MATCH,)], b"999999999\n")],
    "twenty_tokens_ten_numeric": [TWENTY, TWENTY_NEXT],
    "empty_lines": [([], b"\n"), ([], b"\n")],
    "empty_line_behind_a_line": [A12, ([], b"\n")],
}


def valid():
    """{name: (file, text)}"""
    c = {}

    def one(name, m, special=None, **kw):
        b, text = _block(m, special, **kw)
        c[name] = (rc.id_file([b], m), text)
        return b
    for m in (1, 256, 257, 511):                                   # (one line: coded although stored is far smaller)
        one("another_rule_m%d" % m, m)
    for k, (name, pair) in enumerate(sorted(VALID_PAIRS.items())):
        m = (257, 511)[k % 2]
        one("%s_m%d" % (name, m), m, {0: pair, 100: pair})
    one("most_frequent_symbol_f1_m511", 511, norm=_starved)
    # the op of the first token: MATCH is nearly every symbol of row op[0] behind the first line and has 1 of 4096, STR 4095
    b, _ = _block(511)
    rows = dict(b.rows)
    rows[0] = [1, 0, 0, 4095, 0]
    one("f4095_beside_f1_m511", 511, rows=rows)
    # rows with symbols that never occur and have a frequency, and rows 15, 23 and 123 present and never used
    rows = {r: [f - (f > 300) * 200 for f in row] for r, row in b.rows.items()}
    for r, row in rows.items():
        row[2 if r < 16 else 77] += 4096 - sum(row)
    rows[15], rows[23], rows[123] = [819, 819, 819, 819, 820], [16] * 256, [4096] + [0] * 95
    one("frequencies_for_symbols_and_rows_that_never_occur_m511", 511, rows=rows)
    # the first state: an empty line is END in op[0] alone, END has 16 of 4096 and the encoder lets no byte leave in front of it: 2^31 and END's cumulative
    special = {s: [([], b"\n")] for s in range(0, 256, 2)}
    special.update({s: [([(STR, b"a")], b"a\n")] for s in range(1, 256, 2)})
    b = one("first_state_2_31_m256", 256, special, rows={0: [0, 0, 0, 4080, 16], 1: [0, 0, 0, 0, 4096], 28: [0] * 66 + [4096] + [0] * 29, 94: [4096] + [0] * 95},
            lazy_first={s: True for s in range(0, 256, 2)})
    assert any(int.from_bytes(s[:4], "big") >= 1 << 31 for s in b.strands)
    # three blocks through the header's RB, a stored one between coded ones
    blocks = [_block(257, {0: VALID_PAIRS["delta_255"]}), _block(257, stored=True), _block(1)]
    c["three_blocks_middle_stored_n515"] = (rc.id_file([b for b, _ in blocks], 257), b"".join(t for _, t in blocks))
    return c


X = b"?\n"                                                          # a declared line of a strand that is refused before the declaration matters
PREV_PAIRS = {
    "match_on_a_strands_first_line": [([(MATCH,)], X), ([], b"\n")],
    "match_at_a_token_the_previous_line_does_not_have": [([(STR, b"a")], b"a\n"), ([(MATCH,), (MATCH,)], b"a?\n")],
    "delta_against_a_string_token": [([(STR, b"a")], b"a\n"), ([(DELTA, 1)], X)],
    "delta_against_007": [([(STR, b"007")], b"007\n"), ([(DELTA, 1)], b"008\n")],
    "delta_against_ten_digits": [([(STR, b"1234567890")], b"1234567890\n"), ([(DELTA, 1)], b"1234567891\n")],
    "delta_on_a_strands_first_line": [([(DELTA, 1)], X), ([], b"\n")],
}
VALUE_PAIRS = {
    "delta_0": [([(NUM, 5)], b"5\n"), ([(DELTA, 0)], b"5\n")],
    "delta_from_999999900_by_100": [([(NUM, 999999900)], b"999999900\n"), ([(DELTA, 100)], b"1000000000\n")],
    "num_1000000000": [([(NUM, 1000000000)], b"1000000000\n"), ([], b"\n")],
    "num_0xFFFFFFFF": [([(NUM, 0xFFFFFFFF)], b"4294967295\n"), ([], b"\n")],
}
# the lines that the ops write, and by how much the strand's declared text bytes differ from them: each overruns them by exactly one byte, or ends one short
TEXT_PAIRS = {
    "literal_byte_one_past": ([([(STR, b"abc")], b"abc\n"), ([], b"\n")], -3),
    "match_copy_one_past": ([([(STR, b"abc")], b"abc\n"), ([(MATCH,)], b"abc\n")], -2),
    "digits_one_past": ([([(STR, b"a")], b"a\n"), ([(NUM, 12345)], b"12345\n")], -2),
    "newline_one_past": ([([(STR, b"abc")], b"abc\n"), ([], b"\n")], -2),
    "last_newline_one_past": ([([(STR, b"abc")], b"abc\n"), ([(MATCH,)], b"abc\n")], -1),
    "lines_end_one_byte_short": ([([(STR, b"abc")], b"abc\n"), ([(MATCH,)], b"abc\n")], 1),
}


def refusals():
    """{name: (file, (block, code))}"""
    c = {}

    def one(name, code, change=None, m=511, special=None, **kw):
        b, _ = _block(m, special, **kw)
        r = change(b) if change else None
        c[name] = (rc.id_file([b if r is None else r], m, n=m, text_bytes=b.text_bytes), (0, code))

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

    def declare(s, d, total=True):
        """strand s declares d text bytes more; total: block_text_bytes and the file's text_bytes follow"""
        def change(b):
            b.stext[s] += d
            if total:
                b.text_bytes += d
        return change

    def both(*changes):
        def change(b):
            for ch in changes:
                ch(b)
        return change
    spare, low_state = (lambda d: d + b"\0"), (lambda d: b"\x00\x7f\xff\xff" + d[4:])

    def cut_last(d):
        assert len(d) > 4                                          # a renormalisation byte goes, not one of the state
        return d[:-1]

    def body(f):
        def change(b):
            b.body = f(b.body)
        return change
    # ---- one violation each
    one("mode_2", MODE, setter(mode=2))
    one("mode_255", MODE, setter(mode=255))
    one("stored_payload_plus_1", SIZE, raw(add=b"\n"), stored=True)
    one("stored_payload_minus_1", SIZE, raw(cut=-1), stored=True)
    one("payload_ends_in_the_bitmap", SIZE, raw(cut=5 + 2048 + 15))
    one("payload_ends_in_the_table", SIZE, raw(cut=5 + 2048 + 16 + 9))
    one("strand_text_sum_plus_1", SIZE, declare(3, 1, total=False))
    one("strand_text_sum_minus_1", SIZE, declare(3, -1, total=False))
    one("bitmap_bit_124", BITMAP, lambda b: setattr(b, "bitmap", sum(1 << r for r in b.rows) | 1 << 124))
    one("bitmap_bit_127", BITMAP, lambda b: setattr(b, "bitmap", sum(1 << r for r in b.rows) | 1 << 127))
    one("row_sum_4095", ROW, row(0, 3, -1))
    one("row_sum_4097", ROW, row(25, 0, 1))
    one("present_row_all_zero", ROW, lambda b: b.rows.__setitem__(17, [0] * 256))
    one("length_sum_plus_1", LENGTHS, strand(7, length=lambda n: n + 1))
    one("length_sum_minus_1", LENGTHS, strand(7, length=lambda n: n - 1))
    one("payload_bytes_plus_1", LENGTHS, raw(add=b"\0"))
    one("payload_bytes_minus_1", LENGTHS, raw(cut=-1))
    one("strand_with_lines_of_3_bytes", SHORT, strand(9, data=lambda d: d[:3]))
    one("strand_with_fewer_text_bytes_than_lines", SHORT, both(declare(9, -1 - len(_filler(9, 0)[1] + _filler(9, 1)[1]) + 2), declare(10, len(_filler(9, 0)[1] + _filler(9, 1)[1]) - 1)))
    one("strand_without_lines_of_4_bytes", SHORT, strand(200, data=lambda d: rc.LOW.to_bytes(4, "big")), m=257)
    one("strand_without_lines_of_1_text_byte", SHORT, both(declare(200, 1), declare(0, -1)), m=257)
    one("last_byte_removed", TRUNC, strand(3, data=cut_last))
    one("used_row_absent", CONTEXT, drop_row(17))
    one("start_state_2_23_plus_1", END, m=511, start={5: rc.LOW + 1})
    one("spare_byte_behind_a_strand", END, strand(6, data=spare))
    one("first_state_below_2_23", END, strand(2, data=low_state))
    for name, pair in PREV_PAIRS.items():
        one(name, PREV, special={4: pair})
    for name, pair in VALUE_PAIRS.items():
        one(name, VALUE, special={4: pair})
    for name, (pair, d) in TEXT_PAIRS.items():
        one(name, TEXT, declare(4, d), special={4: pair})
    one("newline_one_past_in_the_last_strand", TEXT, declare(255, -1), special={255: [([(STR, b"abc")], b"abc\n")]})
    one("stored_with_one_newline_too_few", TEXT, body(lambda t: t[:9] + t[9:].replace(b"\n", b" ", 1)), stored=True)
    one("stored_with_one_newline_too_many", TEXT, body(lambda t: t[:9] + t[9:].replace(b"x", b"\n", 1)), stored=True)
    one("stored_whose_last_byte_is_no_newline", TEXT, body(lambda t: b"\n" + t[:-1]), stored=True)
    one("str_followed_at_once_by_symbol_0", EMPTY, special={4: [([(STR, b"")], X), ([], b"\n")]})
    # ---- two violations: the smallest code
    one("bad_row_and_short_strand", ROW, both(row(0, 3, 1), strand(9, data=lambda d: d[:3])))
    one("strand_0_truncated_strand_1_wrong_end", TRUNC, strand(0, data=cut_last), start={1: rc.LOW + 1})
    one("strand_0_wrong_end_strand_1_truncated", TRUNC, strand(1, data=cut_last), start={0: rc.LOW + 1})
    one("short_strand_and_wrong_length_sum", LENGTHS, strand(9, length=lambda n: 3))
    one("wrong_text_sum_and_bad_row", SIZE, both(declare(3, 1, total=False), row(0, 3, 1)))
    one("value_in_strand_0_and_prev_in_strand_1", PREV, special={0: VALUE_PAIRS["delta_0"], 1: PREV_PAIRS["delta_against_007"]})
    one("empty_in_strand_0_and_text_in_strand_1", TEXT, declare(1, -3), special={0: [([(STR, b"")], X), ([], b"\n")], 1: TEXT_PAIRS["literal_byte_one_past"][0]})
    one("wrong_end_in_strand_0_and_text_in_strand_200", END, both(strand(0, data=spare), declare(200, 1)), special={200: TEXT_PAIRS["lines_end_one_byte_short"][0]})
    # ---- three blocks: the lowest damaged block, and there the smallest code
    def three(name, want, *changes):
        blocks = [_block(257)[0], _block(257, {0: VALID_PAIRS["delta_255"]})[0], _block(257)[0]]
        for b, ch in zip(blocks, changes):
            if ch:
                ch(b)
        c[name] = (rc.id_file(blocks, 257), want)
    three("blocks_1_and_2_damaged", (1, END), None, strand(4, data=spare), setter(mode=2))
    three("block_2_damaged", (2, ROW), None, None, row(0, 3, -1))
    three("block_1_twice_and_block_2", (1, ROW), None, both(strand(0, data=spare), row(0, 3, 1)), drop_row(17))
    return c


def check_edges():
    """the condition on the valid cases: the decoder written from the README meets a slot at the low and at the high edge of a symbol's range and a step that
    reads two renormalisation bytes, and reads every case back"""
    from tests import readme_decoders as rd
    seen = dict.fromkeys(rd.SEEN, 0)
    rd.SEEN.update(seen)
    for name, (f, text) in sorted(valid().items()):
        assert rd.id_decode(f)[0] == text, name
    seen.update(rd.SEEN)
    assert all(seen.values()), seen
    return seen
