"""Packed quality files that the library's encoder never writes, built to order by tests/rans_craft.py from the README's format text: valid ones with their text,
and damaged ones with the block and the QV_E_* code that the README's rule gives -- written down here by hand, never computed by the decoder under test.
Shared by tests/test_craft_host.py (the sanitizer build and the host twin) and tests/test_gpu_craft.py (the kernel)."""
import random

from tests import rans_craft as rc

MODE, SIZE, ALPHABET, ROW, LENGTHS, SHORT, TRUNC, CONTEXT, END = range(1, 10)
CODES = set(range(1, 10))                                          # the enum of qv_block.h


def _lines(m, L, alphabet, seed, weights=None):
    rng = random.Random(seed)
    return [bytes(rng.choices(alphabet, weights, k=L)) for _ in range(m)]


def _text(lines):
    return b"".join(ln + b"\n" for ln in lines)


def _starved(counts):
    """the most frequent symbol of the row gets 1, and the lowest other symbol of the alphabet -- whether it occurs or not -- what is left after a 1 for every other
    occurring symbol"""
    if not sum(counts):
        return [0] * len(counts)
    top = max(range(len(counts)), key=lambda y: counts[y])
    f = [1 if c else 0 for c in counts]
    other = next(y for y in range(len(counts)) if y != top)
    f[other] += 4096 - sum(f)
    return f


def valid():
    """{name: (file, text)}"""
    c = {}

    def one(name, lines, L, **kw):
        b = rc.QualityBlock(lines, L, **kw)
        c[name] = (rc.quality_file([b], L, len(lines)), _text(lines))
        return b
    one("another_rule_L37_m257", _lines(257, 37, b"#5I", 1, [1, 3, 9]), 37)
    one("another_rule_L2_m513", _lines(513, 2, b"#5I", 2, [1, 3, 9]), 2)
    one("another_rule_L1_m255", _lines(255, 1, b"#5I", 3), 1)
    one("most_frequent_symbol_f1_L2_m256", _lines(256, 2, b"#5I", 4, [1, 2, 30]), 2, norm=_starved)
    # I is one symbol in forty and has 1 of 4096: twelve bits, two renormalisation bytes in a step
    lines = _lines(513, 37, b"5I", 5, [40, 1])
    one("f4095_beside_f1_L37_m513", lines, 37, rows=[[4095, 1]] * 3)
    # seven symbols in the bitmap, the first, the middle and the last never occur and have no frequency; one line, so stored would be far smaller
    lines = _lines(1, 37, b"+5?I", 6)
    one("zero_frequencies_and_coded_where_stored_is_smaller_L37_m1", lines, 37, alphabet=b"!+5:?IK")
    # '~' is in the bitmap, never occurs, has a frequency in every used row and a full row of its own as a context
    lines = _lines(256, 2, b"#5I", 7)
    b = rc.QualityBlock(lines, 2, alphabet=b"#5I~")
    rows = [[f - (f > 300) * 200 for f in r[:3]] + [200 * sum(f > 300 for f in r[:3])] if sum(r) else r for r in b.rows]
    rows[3] = [1000, 1000, 1000, 1096]
    assert all(sum(r) in (0, 4096) for r in rows)
    one("rows_for_a_context_that_never_occurs_L2_m256", lines, 2, alphabet=b"#5I~", rows=rows)
    one("A1_L37_m255", [b"I" * 37] * 255, 37)
    one("A94_L2_m257", _lines(257, 2, bytes(range(33, 127)), 8), 2, alphabet=bytes(range(33, 127)))
    # the first state: the only symbol of a strand has 16 of 4096, and the encoder lets no byte leave in front of it: 2^31 and the symbol's cumulative
    b = one("first_state_2_31_L1_m256", _lines(256, 1, b"5I", 9), 1, rows=[[0, 0], [0, 0], [16, 4080]], start=rc.LOW, lazy_first={s: True for s in range(0, 256, 2)})
    assert any(int.from_bytes(s[:4], "big") >= 1 << 31 for s in b.strands)
    # ... and of a strand of two symbols: the second has all 4096 of its row and leaves the state at 2^23
    b = one("first_state_2_31_L2_m1", [b"5I"], 2, rows=[[0, 4096], [0, 0], [16, 4080]], lazy_first=True)
    assert int.from_bytes(b.strands[0][:4], "big") >= 1 << 31
    # three blocks through the header's RB, the middle one stored
    lines = _lines(513, 2, b"#5I", 10)
    blocks = [rc.QualityBlock(lines[:256], 2), rc.QualityBlock(lines[256:512], 2, stored=True), rc.QualityBlock(lines[512:], 2)]
    c["three_blocks_middle_stored_L2_n513"] = (rc.quality_file(blocks, 2, 256), _text(lines))
    return c


def refusals():
    """{name: (file, (block, code))}"""
    c = {}

    def one(name, code, change, m=257, L=37, seed=20, **kw):
        b = rc.QualityBlock(_lines(m, L, b"#5I", seed, [1, 3, 9]), L, **kw)
        r = change(b)
        c[name] = (rc.quality_file([b if r is None else r], L, m, n=m), (0, code))

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
    spare, low_state = (lambda d: d + b"\0"), (lambda d: b"\x00\x7f\xff\xff" + d[4:])

    def cut_last(d):
        assert len(d) > 4                                          # a renormalisation byte goes, not one of the state
        return d[:-1]
    # ---- one violation each
    one("mode_2", MODE, setter(mode=2))
    one("mode_255", MODE, setter(mode=255))
    one("stored_payload_plus_1", SIZE, raw(add=b"I"), stored=True)
    one("stored_payload_minus_1", SIZE, raw(cut=-1), stored=True)
    one("coded_payload_of_13_bytes", SIZE, raw(cut=13))
    one("coded_payload_without_its_last_length", SIZE, raw(cut=14 + 24 + 1023))
    one("A_0", ALPHABET, setter(A=0))
    one("A_95", ALPHABET, setter(A=95))
    one("A_is_not_the_bitmaps_count", ALPHABET, setter(A=4))
    one("bitmap_bit_94", ALPHABET, lambda b: setattr(b, "bitmap", b.bitmap | 1 << 94))
    one("row_sum_4095", ROW, row(3, 2, -1))
    one("row_sum_4097", ROW, row(0, 1, 1))
    one("length_sum_plus_1", LENGTHS, strand(7, length=lambda n: n + 1))
    one("length_sum_minus_1", LENGTHS, strand(7, length=lambda n: n - 1))
    one("payload_bytes_plus_1", LENGTHS, raw(add=b"\0"))
    one("payload_bytes_minus_1", LENGTHS, raw(cut=-1))
    one("length_above_the_payload", LENGTHS, strand(255, length=lambda n: 0xFFFFFFF0))
    one("strand_with_lines_of_3_bytes", SHORT, strand(9, data=lambda d: d[:3]))
    one("strand_with_lines_of_0_bytes", SHORT, strand(0, data=lambda d: b""))
    one("strand_without_lines_of_4_bytes", SHORT, strand(255, data=lambda d: rc.LOW.to_bytes(4, "big")), m=255)
    one("strand_without_lines_of_1_byte", SHORT, strand(200, data=lambda d: b"\0"), m=1)
    one("last_byte_removed", TRUNC, strand(3, data=cut_last))
    one("last_byte_removed_last_strand", TRUNC, strand(255, data=cut_last))
    one("used_row_zeroed", CONTEXT, lambda b: b.rows.__setitem__(3, [0, 0, 0]))
    one("start_state_2_23_plus_1", END, lambda b: None, start={5: rc.LOW + 1})
    one("spare_byte_behind_a_strand", END, strand(6, data=spare))
    one("first_state_below_2_23", END, strand(2, data=low_state))
    # ---- two violations: the smallest code
    one("bad_row_and_short_strand", ROW, both(row(1, 0, 1), strand(9, data=lambda d: d[:3])))
    one("strand_0_truncated_strand_1_wrong_end", TRUNC, strand(0, data=cut_last), start={1: rc.LOW + 1})
    one("strand_0_wrong_end_strand_1_truncated", TRUNC, strand(1, data=cut_last), start={0: rc.LOW + 1})
    one("short_strand_and_wrong_length_sum", LENGTHS, strand(9, length=lambda n: 3))
    one("used_row_zeroed_and_spare_byte", CONTEXT, both(strand(0, data=spare), lambda b: b.rows.__setitem__(3, [0, 0, 0])))
    # ---- three blocks: the lowest damaged block, and there the smallest code
    def three(name, want, *changes):
        lines = _lines(771, 2, b"#5I", 30, [1, 3, 9])
        blocks = [rc.QualityBlock(lines[a:a + 257], 2) for a in (0, 257, 514)]
        for b, ch in zip(blocks, changes):
            if ch:
                ch(b)
        c[name] = (rc.quality_file(blocks, 2, 257), want)
    three("blocks_1_and_2_damaged", (1, END), None, strand(4, data=spare), setter(mode=2))
    three("block_2_damaged", (2, ROW), None, None, row(3, 0, -1))
    three("block_1_twice_and_block_2", (1, ROW), None, both(strand(0, data=spare), row(3, 1, 1)), setter(A=0))
    return c


def check_edges():
    """the condition on the valid cases: the decoder written from the README meets a slot at the low and at the high edge of a symbol's range and a step that
    reads two renormalisation bytes, and reads every case back"""
    from tests import readme_decoders as rd
    seen = dict.fromkeys(rd.SEEN, 0)
    rd.SEEN.update(seen)
    for name, (f, text) in sorted(valid().items()):
        assert rd.quality_decode(f)[0] == text, name
    seen.update(rd.SEEN)
    assert all(seen.values()), seen
    return seen
