"""The id texts and the pieces that tests/test_gpu_line_walks.py holds the four line-carrying file calls to.  Every text has at most a few dozen lines; `w` is the
width of its regular lines, so that a piece of w + 1 bytes ends on every newline and one of w + 2 bytes a byte behind one."""

W = 11                                                               # "@rNN", five 'x' and "/1"
LONG = 300                                                           # the one long line: a piece of 64 bytes grows over five turns until it holds it
WIDE = 120                                                           # 40 lines of it pass the 4 KiB that a piece of idpack_files never goes below


def _line(i, w=W):
    return (b"@r%02d" % i).ljust(w - 2, b"x") + b"/1"


def text_of(lines):
    return b"".join(l + b"\n" for l in lines)


def texts():
    """name -> (text, w).  A name that ends in "_open": the last line has no newline"""
    even = [_line(i) for i in range(24)]
    long_line = b"@long/1 " + b"y" * (LONG - 8)
    t = {
        "empty": (b"", 0),
        "one_line": (_line(0) + b"\n", W),
        "one_line_open": (_line(0), W),
        "empty_lines": (b"\n" * 5, 0),
        "one_width": (text_of(even), W),
        "long_in_the_middle": (text_of(even[:12] + [long_line] + even[12:]), W),
        "one_width_open": (text_of(even)[:-1], W),
        "wide": (text_of(_line(i, WIDE) for i in range(40)), WIDE),
    }
    assert len(long_line) == LONG and all(len(l) == W for l in even)
    return t


def pieces(w):
    """every piece ends on a newline; a byte behind one; the long line makes the piece grow; larger than any of the files"""
    return sorted({w + 1, w + 2, 64, 1 << 20})


def lines(text):
    """the lines of a text without their newlines; a last line without one counts"""
    if not text:
        return []
    out = text.split(b"\n")
    if text.endswith(b"\n"):
        out.pop()
    return out


def fixed(n, tag):
    """n lines of six characters that tell their record"""
    return b"".join(b"%05d%s\n" % (i, tag) for i in range(n))


def join(ids, dna, quality):
    """the FASTQ text of the three texts: a bare '+' as the third line"""
    d, q = lines(dna), lines(quality)
    return b"".join(i + b"\n" + d[k] + b"\n+\n" + q[k] + b"\n" for k, i in enumerate(lines(ids)))


def name(line):
    """the name of a line of these texts: without the '@', up to the first space, without "/1" """
    n = line[1:].split(b" ")[0]
    return n[:-2] if n.endswith(b"/1") and len(n) >= 3 else n


def listed(ids):
    """a list of names for select_files: every third line's, the last line's, the long line's, and one that no line carries"""
    ls = lines(ids)
    pick = sorted(set(range(0, len(ls), 3)) | {len(ls) - 1} | {k for k, l in enumerate(ls) if len(l) == LONG}) if ls else []
    return b"".join(name(ls[k]) + b"\n" for k in pick if name(ls[k])) + b"nobody\n"


def mates(ids):
    """two partner texts for idmate_rule_files: the ids of the mates under the rule slash, line for line as long as their partners; and short ids of other
    lengths, which fall into the pieces differently and hold no rule"""
    ls = lines(ids)
    return text_of(l.replace(b"/1", b"/2", 1) for l in ls), text_of(b"@%d" % k for k in range(len(ls)))
