"""The host twins of the mate rule (harc_amd_idmate_rule_host / harc_amd_idmate_apply_host, harc_amd/csrc/idmate.h) against the Python restatement of
tests/idmate_cases.py, without a GPU; and what folding the second file's ids away saves, measured on 20 000 Illumina-style pairs."""
import pytest

import harc_amd
from tests import idmate_cases as mc

CASES = mc.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_rule_host_equals_the_restatement(name):
    a, b = CASES[name]
    want_flags, want_rule = mc.flags_and(a, b), mc.rule(a, b)
    got_rule, pairs, flags = harc_amd.idmate_rule_host(a, b)
    assert (got_rule, pairs, flags) == (want_rule, len(mc.lines(a)), want_flags), name
    if want_rule != "none":                                        # by construction: folding is lossless without a second check
        made, bad = harc_amd.idmate_apply_host(a, want_rule)
        assert made == b and bad == 0, name
        assert mc.apply(a, want_rule) == (b, 0)


def test_every_rule_and_none_occur_among_the_cases():
    seen = {mc.rule(a, b) for a, b in CASES.values()}
    assert seen == set(mc.RULES), seen
    # a pair satisfies at most one rule
    for a, b in CASES.values():
        for x, y in zip(mc.lines(a), mc.lines(b)):
            assert mc.pair_flags(x, y) in (0, mc.SAME, mc.SLASH, mc.SPACE), (x, y)


@pytest.mark.parametrize("r", ["slash", "space", "same", "none"])
def test_apply_host_counts_exactly_the_lines_without_the_1(r):
    for name, text in mc.apply_cases().items():
        want, want_bad = mc.apply(text, r)
        got, bad = harc_amd.idmate_apply_host(text, r)
        assert (got, bad) == (want, want_bad), (name, r)
    if r in ("slash", "space"):
        assert mc.apply(mc.apply_cases()["no_space_anywhere"], r)[1] > 0


def test_apply_host_leaves_an_open_last_line_alone():
    got, bad = harc_amd.idmate_apply_host(b"@a/1\n@b/1", "slash")
    assert (got, bad) == (b"@a/2\n@b/1", 0)


def test_unequal_line_counts_and_an_open_last_line_are_refused():
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.idmate_rule_host(b"@a\n@b\n@c\n", b"@a\n@b\n")
    assert e.value.code == -1 and "3 lines" in str(e.value) and " 2" in str(e.value)
    for a, b in ((b"@a\n@b", b"@a\n@b\n"), (b"@a\n@b\n", b"@a\n@b"), (b"@a", b"@a")):
        with pytest.raises(harc_amd.HarcAmdError) as e:
            harc_amd.idmate_rule_host(a, b)
        assert e.value.code == -1 and "no newline" in str(e.value)
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.idmate_apply_host(b"@a/1\n", 7)
    assert harc_amd.idmate_rule_host(b"", b"") == ("same", 0, 7)
    assert harc_amd.build_has("pair")


def test_size_table_of_folded_ids(capsys):
    """X.id and idpack_host(X.id) on 20 000 Illumina-style pairs, folded (file 1's ids) and unfolded (the cat layout: file 1's ids, then file 2's).
    The table is README.md's ("-2 and what it promises")."""
    a, b = mc.illumina_pairs(20000)
    ta, tb = mc.text_of(a), mc.text_of(b)
    assert harc_amd.idmate_rule_host(ta, tb)[0] == "space"
    folded, unfolded = ta, ta + tb
    hi_f, hi_u = harc_amd.idpack_host(folded), harc_amd.idpack_host(unfolded)
    with capsys.disabled():
        print("\n20 000 pairs of ids       X.id bytes   X.id.hi bytes")
        print("unfolded (cat layout)   %12d   %13d" % (len(unfolded), len(hi_u)))
        print("folded (-2)             %12d   %13d" % (len(folded), len(hi_f)))
    assert 2 * len(folded) == len(unfolded)
    assert harc_amd.idunpack_host(hi_f) == folded
    assert len(hi_f) < len(hi_u)
