"""Inputs of the range restore (./harc -d -r FIRST:LAST), shared by the host test, the script test and the GPU test, and the contract in plain Python:
slice_lines says which bytes of a text a range of lines is, line_offset what the line select of harc_amd/csrc/linesel.h answers.  Lines are counted from 0
here, as in the library; ./harc -r counts from 1."""
import random

NONE = 2 ** 64 - 1


def lines_of(text):
    """the closed lines of a text, newlines included: a last line without its newline is not one"""
    parts = text.split(b"\n")
    return [p + b"\n" for p in parts[:-1]]


def slice_lines(text, first, count):
    """lines first .. first + count - 1 of `text`: what a range restore writes"""
    return b"".join(lines_of(text)[first:first + count])


def slice_records(fastq, first, count):
    """records first .. first + count - 1 of a FASTQ text of 4-line records"""
    return slice_lines(fastq, 4 * first, 4 * count)


def line_offset(text, k):
    """(newlines of text, where line k starts: 0 for k = 0, else one past the k-th newline, NONE when there are fewer), by bytes.split"""
    parts = text.split(b"\n")
    nl = len(parts) - 1
    if k == 0:
        return nl, 0
    if k > nl:
        return nl, NONE
    return nl, sum(len(p) + 1 for p in parts[:k])


def ks(text):
    """the line numbers every text is asked for: the first line, the second, the end of the last, and one that is not there"""
    nl = text.count(b"\n")
    return sorted({0, 1, nl, nl + 1})


def _filler(n, seed, every=11):
    """n bytes of id-like characters with a newline about every `every` bytes"""
    rng = random.Random(seed)
    return bytes(10 if rng.randrange(every) == 0 else rng.choice(b"@SRR.0123456789:HWI length=") for _ in range(n))


def texts():
    """{name: text}: the sizes at which a 16-byte chunk, a row of 256 chunks and a workgroup's span begin and end, and the places a newline can sit"""
    out = {}
    for n in (0, 1, 15, 16, 17, 4095, 4096, 4097):
        out["filler_%d" % n] = _filler(n, 100 + n)
    out["newline_alone"] = b"\n"
    out["newline_first"] = b"\n" + _filler(40, 1, every=1000).replace(b"\n", b"x")
    out["newline_last"] = _filler(40, 2, every=1000).replace(b"\n", b"x") + b"\n"
    out["newline_first_and_last"] = b"\n" + b"abc" * 11 + b"\n"
    out["no_newline"] = _filler(5000, 3, every=10 ** 9).replace(b"\n", b"x")
    out["newlines_200"] = b"\n" * 200                              # a wave's span of 64 chunks holds more than 64 newlines
    out["newlines_200_inside"] = b"@id" * 700 + b"\n" * 200 + b"@id" * 900 + b"\n"
    out["newlines_5000"] = b"\n" * 5000                            # more than one row of chunks, every bit of every mask set
    return out


def id_like(nbytes=1 << 20, seed=23):
    """about nbytes of lines as a sequencer names its reads, every one closed"""
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < nbytes:
        i += 1
        line = b"@SRR870667.%d HWI-ST1234:100:C0ABCACXX:3:%d:%d:%d length=100\n" % (i, 1101 + i // 5000, rng.randrange(1000, 20000), rng.randrange(1000, 200000))
        out.append(line)
        size += len(line)
    return b"".join(out)


def lines_of_lengths(lengths, seed=5):
    """closed lines of exactly these lengths (newline not counted)"""
    rng = random.Random(seed)
    return b"".join(bytes(rng.choice(b"abcdefgh") for _ in range(n)) + b"\n" for n in lengths)
