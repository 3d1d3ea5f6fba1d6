"""The host twin of the rule of the third lines (harc_amd_third_rule_host, harc_amd/csrc/third.h) against the rule restated in Python (tests/third_cases.py),
on every edge the issue names; the names and numbers of the rules in both directions.  No device."""
import pytest

from tests import third_cases as tc

CASES = tc.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_the_python_rule(name):
    import harc_amd
    txt = CASES[name]
    f, n = tc.text_flags(txt)
    assert tc.rule_of(f, n) == tc.EXPECTED[name]                   # the case is what its name says
    assert harc_amd.third_rule_host(txt) == (tc.EXPECTED[name], n, f)


def test_the_cases_cover_every_rule_and_both_flags_at_once():
    got = {tc.text_flags(t) for t in CASES.values()}
    assert {f for f, n in got if n} == {0, tc.BARE, tc.SAME, tc.BARE | tc.SAME}
    assert set(tc.EXPECTED.values()) == {"bare", "same", "dropped"}


@pytest.mark.parametrize("k", range(0, 41))
def test_host_twin_on_lines_of_every_length(k):
    import harc_amd
    txt = tc.alignment_text(k)
    f, n = tc.text_flags(txt)
    assert n == 16 and f == (0 if k == 0 else tc.BARE | tc.SAME if k == 1 else tc.SAME)
    assert harc_amd.third_rule_host(txt)[1:] == (n, f)
    for byte in sorted({0, 1, k // 2, k - 1} & set(range(k))):
        bad = tc.alignment_text(k, broken=(k % 16, byte))
        assert tc.text_flags(bad) == (0, 16) and harc_amd.third_rule_host(bad) == ("dropped", 16, 0), (k, byte)


def test_names_and_numbers_of_the_rules():
    import harc_amd
    assert harc_amd.THIRD_RULES == ("dropped", "bare", "same")
    for number, name in enumerate(harc_amd.THIRD_RULES):
        assert harc_amd.third_rule_name(number) == name and harc_amd.third_rule_parse(name) == number
    for bad in (-1, 3, 100):
        assert harc_amd.third_rule_name(bad) == "?"
    for bad in ("", "Same", "same ", "none", "?", "bare\n"):
        assert harc_amd.third_rule_parse(bad) == -1
    # the rule of a flag word: no record gives bare whatever the word, the bare bit wins, then the same bit
    for f in range(4):
        assert harc_amd.third_rule_of(f, 0) == "bare"
        assert harc_amd.third_rule_of(f, 5) == tc.rule_of(f, 5)
    assert [harc_amd.third_rule_of(f, 1) for f in range(4)] == ["dropped", "bare", "same", "bare"]


def test_header_and_third_h_agree_on_the_numbers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "harc_amd.h")).read()
    th = open(os.path.join(root, "harc_amd", "csrc", "third.h")).read()
    for name in ("DROPPED", "BARE", "SAME"):
        a = re.search(r"#define HARC_AMD_THIRD_%s (\d+)" % name, hdr).group(1)
        b = re.search(r"#define TH_%s (\d+)" % name, th).group(1)
        assert a == b
