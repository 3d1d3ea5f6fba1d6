"""The mate rule of paired-end ids restated in plain Python (README: "-2 and what it promises"), and the id sets the host twins and the kernels are held to.
a = id line i of file 1, b = id line i of file 2, without their newlines.  A pair satisfies at most one of
  same   b == a
  slash  |a| = |b| >= 2, a ends in /1, b is a with its last byte 2
  space  |a| = |b|, a has a first space at s with s + 1 < |a|, a[s + 1] = '1', b is a with byte s + 1 set to '2'
The rule of two files is the one every pair satisfies; no pair gives same; otherwise none.  Test infrastructure only."""
import functools
import random

from tests import bgzf_out_cases

SAME, SLASH, SPACE = 1, 2, 4
RULES = ("none", "same", "slash", "space")


def pair_flags(a, b):
    f = 0
    if a == b:
        f |= SAME
    if len(a) == len(b) >= 2 and a.endswith(b"/1") and b == a[:-1] + b"2":
        f |= SLASH
    s = a.find(b" ")
    if len(a) == len(b) and s >= 0 and s + 1 < len(a) and a[s + 1:s + 2] == b"1" and b == a[:s + 1] + b"2" + a[s + 2:]:
        f |= SPACE
    return f


def lines(text):
    assert text == b"" or text.endswith(b"\n")
    return text.split(b"\n")[:-1]


def flags_and(ta, tb):
    la, lb = lines(ta), lines(tb)
    assert len(la) == len(lb)
    f = SAME | SLASH | SPACE
    for a, b in zip(la, lb):
        f &= pair_flags(a, b)
    return f


def rule(ta, tb):
    n, f = len(lines(ta)), flags_and(ta, tb)
    if n == 0:
        return "same"
    return "same" if f & SAME else "slash" if f & SLASH else "space" if f & SPACE else "none"


def apply(text, r):
    """-> (file 2's ids from file 1's, the lines that did not carry the '1' to replace: they stay as they are)"""
    if r in ("same", "none"):
        return text, 0
    out, bad = [], 0
    for a in lines(text):
        if r == "slash":
            p = len(a) - 1 if a else -1
        else:
            s = a.find(b" ")
            p = s + 1 if s >= 0 and s + 1 < len(a) else -1
        if p < 0 or a[p:p + 1] != b"1":
            bad += 1
            out.append(a)
        else:
            out.append(a[:p] + b"2" + a[p + 1:])
    return b"".join(x + b"\n" for x in out), bad


def text_of(ids):
    return b"".join(x + b"\n" for x in ids)


@functools.lru_cache(maxsize=None)
def illumina_pairs(n, seed=11):
    """(ids of file 1, ids of file 2) in the Illumina 1.8 style, the instrument fields taken from the ids of bgzf_out_cases.illumina_text:
    @HWI-ST1234:100:C0ABCACXX:3:<tile>:<x>:<y> 1:N:0:ATCACG and ... 2:N:0:ATCACG"""
    ids = bgzf_out_cases.illumina_text(n, seed).split(b"\n")[0::4][:n]
    core = [b"@" + x.split(b" ")[1] for x in ids]
    return tuple(c + b" 1:N:0:ATCACG" for c in core), tuple(c + b" 2:N:0:ATCACG" for c in core)


def slash_pairs(n, seed=11):
    a, _ = illumina_pairs(n, seed)
    core = [x.split(b" ")[0] for x in a]
    return tuple(c + b"/1" for c in core), tuple(c + b"/2" for c in core)


def sra_pairs(n, seed=11):
    ids = tuple(bgzf_out_cases.illumina_text(n, seed).split(b"\n")[0::4][:n])
    return ids, ids


def _line_of(k, tail):
    """k bytes that end in `tail`, '@' first where there is room"""
    body = (b"@" + b"abcdefghijklmnopqrstuvwxyz0123456789" * 3)[:max(0, k - len(tail))]
    return (body + tail)[-k:] if k else b""


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (text of file 1's ids, text of file 2's ids)}; every text is closed lines"""
    rng = random.Random(5)
    c = {}
    n = 300
    a, b = illumina_pairs(n)
    c["illumina_space"] = (a, b)
    c["slash"] = slash_pairs(n)
    c["sra_same"] = sra_pairs(n)
    shuffled = list(b)
    rng.shuffle(shuffled)
    c["unpaired_shuffled"] = (a, tuple(shuffled))
    c["space_but_last"] = (a, b[:-1] + (a[-1],))                   # the last pair is identical instead
    sa, sb = slash_pairs(n)
    c["slash_but_first"] = (sa, (sa[0][:-2] + b"x2",) + sb[1:])     # the first pair also differs in front of the digit
    # adversarial lines, each as a set of its own (one pair) and all together
    adv = {
        "several_spaces": (b"@x 1:N 1:N 1", b"@x 2:N 1:N 1"),
        "several_spaces_second_changed": (b"@x 1:N 1:N", b"@x 1:N 2:N"),
        "slash_and_elsewhere": (b"@read7/1", b"@reed7/2"),
        "space_rule_at_last_byte": (b"@x 1", b"@x 2"),
        "space_as_last_byte": (b"@x ", b"@x "),
        "space_as_last_byte_changed": (b"@x1 ", b"@x2 "),
        "slash_without_slash": (b"@x1", b"@x2"),
        "just_1": (b"1", b"2"),
        "slash_min": (b"/1", b"/2"),
        "space_min": (b" 1", b" 2"),
        "slash_after_space": (b"@a b/1", b"@a b/2"),
        "space_then_slash_1": (b"@a 1/1", b"@a 1/2"),
        "space_then_slash_2": (b"@a 1/1", b"@a 2/1"),
        "two_changes": (b"@a 1/1", b"@a 2/2"),
        "digit_other": (b"@a 1:N", b"@a 3:N"),
        "digit_from_other": (b"@a 0:N", b"@a 2:N"),
        "longer_b": (b"@a 1", b"@a 12"),
        "empty_line": (b"", b""),
        "empty_against_one": (b"", b"2"),
    }
    for name, (x, y) in adv.items():
        c["adv_" + name] = ((x,), (y,))
    # the load-width and alignment boundaries: lines of k bytes under each rule, and with a byte broken at the front, in the middle and at the end
    for k in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65):
        same = _line_of(k, b"")
        c["len%d_same" % k] = ((same,) * 3, (same,) * 3)
        if k >= 2:
            x = _line_of(k, b"/1")
            c["len%d_slash" % k] = ((x,) * 3, (x[:-1] + b"2",) * 3)
            y = _line_of(k, b" 1")
            c["len%d_space_end" % k] = ((y,) * 3, (y[:-1] + b"2",) * 3)
        if k >= 4:
            z = b"@ 1" + _line_of(k - 3, b"")[1:] + b"z"
            z = z[:k]
            c["len%d_space_front" % k] = ((z,) * 3, (z[:2] + b"2" + z[3:],) * 3)
            for at in (0, k // 2, k - 1):                           # a second difference somewhere else: no rule
                w = bytearray(z[:2] + b"2" + z[3:])
                if at != 2:
                    w[at] ^= 1
                    c["len%d_space_front_broken_at_%d" % (k, at)] = ((z,) * 3, (bytes(w),) * 3)
    for m in (0, 1, 2, 255, 256, 257):
        a, b = illumina_pairs(257)
        c["n%d_space" % m] = (a[:m], b[:m])
        if m:
            c["n%d_space_but_last" % m] = (a[:m], b[:m - 1] + (b[m - 1][:-1] + b"C",))
    mixed_a = tuple(x for x, _ in adv.values())
    mixed_b = tuple(y for _, y in adv.values())
    c["adv_all_together"] = (mixed_a, mixed_b)
    return {k: (text_of(x), text_of(y)) for k, (x, y) in c.items()}


def apply_cases():
    """texts to patch: every file 1 of cases() and lines that lack the byte to replace"""
    t = {k: v[0] for k, v in cases().items()}
    t["no_space_anywhere"] = text_of([b"@abc", b"", b"1", b"@x 1", b"@x ", b"@y 2:N", b"@z/1", b"/1", b"@longer line without the digit /3"] * 5)
    return t
