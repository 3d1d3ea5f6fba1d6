"""Selection by name (./harc -d -q -L NAMES) restated in plain Python from the rule's text, not from the C++: the name of a line, the flags of an id text
against a list, the gather of the flagged lines, the filter of a FASTQ text; and the cases the host twins and the kernels are held to.

The name of a line (without its newline, any bytes, '\\r' a byte like any other):
  1. a leading '@' is skipped;
  2. the name runs up to, not including, the first space (0x20) or tab (0x09), or to the end of the line;
  3. a name of at least 3 bytes that ends in '/1' or '/2' loses those two bytes, once.
An empty name never matches; list lines with an empty name are skipped; duplicates count once; a last line without its newline counts as a line."""


def lines(text):
    """the lines of a text without their newlines; a last line without one counts"""
    if not text:
        return []
    out = text.split(b"\n")
    if text.endswith(b"\n"):
        out.pop()
    return out


def key(line):
    """the name of a line"""
    if line[:1] == b"@":
        line = line[1:]
    end = len(line)
    for i, b in enumerate(line):
        if b in (0x20, 0x09):
            end = i
            break
    name = line[:end]
    if len(name) >= 3 and name[-2:] in (b"/1", b"/2"):
        name = name[:-2]
    return name


def key_span(line):
    """(offset, length) of the name inside the line"""
    return (1 if line[:1] == b"@" else 0), len(key(line))


def name_set(names):
    return {key(l) for l in lines(names)} - {b""}


def flags(names, ids):
    """one byte per id line: 1 when its name is listed"""
    s = name_set(names)
    return bytes(1 if key(l) in s else 0 for l in lines(ids))


def counts(names, ids):
    """(distinct names, names found)"""
    s = name_set(names)
    return len(s), len(s & {key(l) for l in lines(ids)})


def missing(names, ids, most=10):
    """the listed names that no id line carries, in list order, each once"""
    have = {key(l) for l in lines(ids)}
    out = []
    for l in lines(names):
        k = key(l)
        if k and k not in have and k not in out:
            out.append(k)
    return out[:most]


def gather(text, f, stride=0):
    """the flagged lines of a text: of `stride` bytes each, or (stride 0) of any length with their newlines (a last line without one as it is)"""
    if stride:
        assert len(text) == stride * len(f)
        return b"".join(text[i * stride:(i + 1) * stride] for i in range(len(f)) if f[i])
    ls = text.split(b"\n")
    parts = [l + b"\n" for l in ls[:-1]] + ([ls[-1]] if ls[-1] else [])
    assert len(parts) == len(f)
    return b"".join(p for p, x in zip(parts, f) if x)


def select_fastq(fastq, names, also=None):
    """the 4-line records of a FASTQ text whose id line carries a listed name; also: per-record flags ORed in (the mate's)"""
    ls = fastq.split(b"\n")
    assert ls[-1] == b"" and (len(ls) - 1) % 4 == 0
    s = name_set(names)
    out = []
    for r in range((len(ls) - 1) // 4):
        if key(ls[4 * r]) in s or (also is not None and also[r]):
            out += ls[4 * r:4 * r + 4]
    return b"".join(l + b"\n" for l in out)


def fastq_flags(fastq, names):
    return flags(names, b"".join(l + b"\n" for l in fastq.split(b"\n")[:-1][0::4]))


# ---- the cases
NAME_LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)


def _name(n, salt=0):
    """n bytes that hold no space, tab, '@' or '/' and do not end in a digit"""
    return bytes(0x41 + (7 * i + 3 * salt + n) % 26 for i in range(n))


def id_lines():
    """id lines: every name length, ended by a space, a tab and the line's end, with and without '@', with and without /1 and /2; the named edge lines; near misses;
    irregular lines"""
    out = []
    for n in NAME_LENGTHS:
        base = _name(n)
        for at in (b"@", b""):
            for tail in (b"", b"/1", b"/2"):
                for end in (b"", b" comment 1:N:0", b"\tx"):
                    out.append(at + base + tail + end)
    out += [b"/1", b"@/1", b"a/1", b"@a/1 x", b"ab/3", b"@ab/3", b"a/1/2", b"@a/1/2\tq", b"a/2/1", b"x/", b"/", b"//1", b"@@x", b"@ @", b"a\r", b"a\r/1", b"a/1\r"]
    # near misses: the last byte, byte 8, byte 64, a prefix
    for n in (9, 65, 70, 129):
        base = bytearray(_name(n, 1))
        for pos in (n - 1, 8, 64):
            if pos < n:
                v = bytearray(base)
                v[pos] = 0x61 + (v[pos] % 26)
                out.append(b"@" + bytes(v))
        out.append(b"@" + bytes(base))
        out.append(b"@" + bytes(base) + b"0")
        out.append(b"@" + bytes(base[:-1]))
    out += [b"r7", b"r70", b"@r7/1 comment", b"r7/2", b"@r7", b"r7 x", b"@r70/1"]
    out += [b"", b"@", b" ", b"\t", b"@ x", b"@\tx", b"", b"@"]
    return out


def _text(ls, open_tail=False):
    t = b"".join(l + b"\n" for l in ls)
    return t[:-1] if open_tail and t else t


def cases():
    """name -> (list of names, id text)"""
    ids = id_lines()
    all_ids = _text(ids)
    names_of = []
    for l in ids:
        k = key(l)
        if k and k not in names_of:
            names_of.append(k)
    some = names_of[::3]
    c = {}
    c["every third name"] = (_text(some), all_ids)
    c["every name"] = (_text(names_of), all_ids)
    c["one name"] = (_text([_name(64)]), all_ids)
    c["no matching name"] = (_text([b"nobody", b"ZZZ/1", _name(64) + b"x"]), all_ids)
    c["duplicates, empty lines, comments, no final newline"] = (_text([b"r7 the first", b"", b"@r7/2", b"r7", b" ", b"@", _name(8) + b"\tcomment", b"@" + _name(8) + b"/1", b"absent",
                                                                       b"absent too", b"absent", _name(300) + b" x"], open_tail=True), all_ids)
    c["list as id lines"] = (_text(ids[::5]), all_ids)
    c["open last id line"] = (_text(some), _text(ids + [b"@" + _name(65) + b"/2 last"], open_tail=True))
    c["open last id line, not listed"] = (_text(some), _text(ids + [b"@nobody"], open_tail=True))
    c["one id line, open"] = (_text([b"a"]), b"@a/1")
    c["one id line"] = (_text([b"a"]), b"@a/1\n")
    c["only empty id lines"] = (_text([b"a"]), b"\n\n\n")
    c["near misses listed"] = (_text([b"r7", _name(9, 1), _name(65, 1), _name(129, 1)[:-1]]), all_ids)
    c["prefix chain"] = (_text([b"A" * n for n in (1, 2, 3, 8, 9, 64, 65)]), _text([b"@" + b"A" * n for n in range(0, 70)]))
    c["carriage returns"] = (b"a\r\nb\r\n", _text([b"@a", b"@a\r", b"@b\r x", b"@b"]))
    return c


def gather_cases():
    """name -> (text, flags, stride)"""
    out = {}
    for stride in (2, 101, 256):
        n = 37
        text = b"".join(bytes(0x21 + (i * 31 + j * 7) % 90 for j in range(stride - 1)) + b"\n" for i in range(n))
        pats = {"nothing": bytes(n), "everything": bytes([1]) * n, "first": bytes([1]) + bytes(n - 1), "last": bytes(n - 1) + bytes([1]),
                "mixed": bytes((i * 5 % 7 < 3) for i in range(n)), "runs": bytes((i // 5) % 2 for i in range(n))}
        for p, f in pats.items():
            out["stride %d, %s" % (stride, p)] = (text, f, stride)
    ids = id_lines()
    for open_tail in (False, True):
        text = _text(ids, open_tail=open_tail)
        n = len(lines(text)) if text else 0
        if open_tail:
            # (the last id line is '@': the open text ends in it)
            assert n == len(ids)
        pats = {"nothing": bytes(n), "everything": bytes([1]) * n, "first": bytes([1]) + bytes(n - 1), "last": bytes(n - 1) + bytes([1]),
                "mixed": bytes((i * 5 % 7 < 3) for i in range(n))}
        for p, f in pats.items():
            out["lines%s, %s" % (" open" if open_tail else "", p)] = (text, f, 0)
    return out
