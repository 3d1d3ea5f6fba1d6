"""The text digest and the record read.check without a GPU: the numpy model is additive over any cut, every single-byte substitution changes D, exchanged lines
change it unless they are equal, the serial host call of the library (check_block.h, the arithmetic the kernel compiles) gives the model's numbers, and the parser
refuses what is no record."""
import random

import pytest

from tests import check_cases as cc


def _text(seed, n):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGTN\n@:0123456789IH#") for _ in range(n))


def test_the_model_is_additive_over_any_cut():
    text = _text(1, 300)
    whole = cc.text_digest(text)
    assert whole[0] == 300 and whole[1] == text.count(b"\n")
    for cut in range(0, 301):
        assert cc.add(cc.text_digest(text[:cut]), cc.text_digest(text[cut:], cut)) == whole, cut
    rng = random.Random(2)
    for _ in range(20):                                            # several pieces, added in any order
        cuts = sorted(rng.sample(range(301), 5))
        pieces = [(a, b) for a, b in zip([0] + cuts, cuts + [300])]
        rng.shuffle(pieces)
        t = (0, 0, 0)
        for a, b in pieces:
            t = cc.add(t, cc.text_digest(text[a:b], a))
        assert t == whole
    assert cc.text_digest(b"") == (0, 0, 0) and cc.text_digest(b"", 77) == (0, 0, 0)
    # the offset counts: the same bytes elsewhere in a text are other terms
    assert cc.text_digest(text, 1)[2] != whole[2] and cc.text_digest(text, 1 << 40)[2] != whole[2]


def test_every_single_byte_substitution_changes_D():
    text = _text(3, 300)
    d = cc.text_digest(text)[2]
    rng = random.Random(4)
    for pos in sorted(set(rng.sample(range(1, 299), 20)) | {0, 299}):
        for v in range(256):
            if v == text[pos]:
                continue
            t = cc.text_digest(text[:pos] + bytes([v]) + text[pos + 1:])
            assert t[0] == 300 and t[2] != d, (pos, v)


def test_exchanged_lines_change_D_unless_they_are_equal():
    lines = [b"ACGTACGT", b"TTTTACGA", b"ACGTACGT", b"GGGGCCCC", b"ACGTACGA"]
    text = b"".join(l + b"\n" for l in lines)

    def swapped(i, j):
        l = list(lines)
        l[i], l[j] = l[j], l[i]
        return b"".join(x + b"\n" for x in l)

    t = cc.text_digest(text)
    for i, j in ((0, 1), (1, 3), (0, 4), (3, 4)):
        u = cc.text_digest(swapped(i, j))
        assert u[:2] == t[:2] and u[2] != t[2], (i, j)
    assert cc.text_digest(swapped(0, 2)) == t
    assert cc.order_digest(lines) == (t[0], t[2])


def test_the_host_call_of_the_library_gives_the_models_numbers():
    import harc_amd
    text = _text(5, 4099)
    for first in (0, 1, (1 << 32) - 5, (1 << 40) + 1):
        for n in (0, 1, 15, 16, 17, 300, 4099):
            assert harc_amd.text_digest_host(text[:n], first) == cc.text_digest(text[:n], first), (first, n)
    # added to what the accumulator holds
    a = harc_amd.text_digest_host(text[:1000])
    assert harc_amd.text_digest_host(text[1000:], 1000, acc=a) == cc.text_digest(text)


def test_the_record_is_written_and_read_back():
    items = {"reads": (3000, 0x1234567890ABCDEF, 7), "order": (303000, 0xFFFFFFFFFFFFFFFF), "ids": (10, 2, 3), "quality": (303000, 3000, 0)}
    data = cc.write_check(items)
    assert data.startswith(b"HARCV1\nreads 0000000000000bb8 1234567890abcdef 0000000000000007\norder ")
    assert cc.parse_check(data) == items
    assert cc.parse_check(cc.write_check({"reads": (0, 0, 0)})) == {"reads": (0, 0, 0)}


@pytest.mark.parametrize("data,named", [
    (b"", "line 1"),
    (b"HARCV2\nreads 0000000000000001 0000000000000002 0000000000000003\n", "line 1"),
    (b"harcv1\nreads 0000000000000001 0000000000000002 0000000000000003\n", "line 1"),
    (b"HARCV1\n", "no line 'reads'"),
    (b"HARCV1\norder 0000000000000001 0000000000000002\n", "no line 'reads'"),
    (b"HARCV1\nreads 0000000000000001 0000000000000002\n", "line 2"),                                          # a value short
    (b"HARCV1\nreads 0000000000000001 0000000000000002 0000000000000003 0000000000000004\n", "line 2"),        # one too many
    (b"HARCV1\nreads 0000000000000001 0000000000000002 000000000000003\n", "line 2"),                          # 15 digits
    (b"HARCV1\nreads 0000000000000001 0000000000000002 000000000000000A\n", "line 2"),                         # upper case
    (b"HARCV1\nreads 0000000000000001 0000000000000002 0000000000000003\nsizes 0000000000000001\n", "line 3"),
    (b"HARCV1\nreads 0000000000000001 0000000000000002 0000000000000003\nquality 0000000000000001 0000000000000002\n", "line 3"),
    (b"HARCV1\nreads 0000000000000001 0000000000000002 0000000000000003\n\nids 0000000000000001 0000000000000002 0000000000000003\n", "line 3"),
    (b"HARCV1\nreads 0000000000000001 0000000000000002 0000000000000003\nreads 0000000000000001 0000000000000002 0000000000000003\n", "line 3"),
])
def test_the_parser_refuses_naming_the_line(data, named):
    with pytest.raises(ValueError) as e:
        cc.parse_check(data)
    assert named in str(e.value), str(e.value)
