"""The rule of the third lines of a FASTQ file (harc_amd/csrc/third.h) restated in a few lines of Python, and the texts the host twin, the kernel and the
stand-alone sanitizer program are held to.  Nothing here calls the code under test."""
import random

BARE, SAME = 1, 2


def record_flags(a, t):
    """a: the id line, t: the third line, without their newlines"""
    f = 0
    if t == b"+":
        f |= BARE
    if len(t) == len(a) >= 1 and t[:1] == b"+" and t[1:] == a[1:]:
        f |= SAME
    return f


def text_flags(txt):
    """-> (the AND of the flags of the records whose third line is there, their number).  Lines as the library counts them: one per newline, and what follows
    the last newline when it is not empty"""
    ls = txt.split(b"\n")
    if ls[-1] == b"":
        ls.pop()
    f, n = BARE | SAME, 0
    for k in range(2, len(ls), 4):
        f &= record_flags(ls[k - 2], ls[k])
        n += 1
    return f, n


def rule_of(f, n):
    return "bare" if n == 0 or f & BARE else "same" if f & SAME else "dropped"


def rule(txt):
    return rule_of(*text_flags(txt))


def record(a, t, L=4, nl=b"\n", seed=0):
    rng = random.Random(seed * 7919 + len(a) * 31 + len(t))
    return a + nl + bytes(rng.choice(b"ACGT") for _ in range(L)) + nl + t + nl + bytes(rng.choice(b"FGHIJ#5") for _ in range(L)) + nl


def sra_id(i, L=100):
    return b"@SRR1234567.%d %d length=%d" % (i, i, L)


def same_file(n, L=4, start=1):
    return [record(sra_id(i, L), b"+" + sra_id(i, L)[1:], L, seed=i) for i in range(start, start + n)]


def cases():
    """name -> FASTQ text; what the rule of each is follows from record_flags alone"""
    c = {}
    c["empty"] = b""
    c["one_same"] = record(b"@id 1", b"+id 1")
    c["one_bare"] = record(b"@id 1", b"+")
    c["id_of_length_1"] = record(b"@", b"+")                       # both flags
    c["id_of_length_1_among_same"] = b"".join(same_file(3)) + record(b"@", b"+") + b"".join(same_file(3, start=9))
    c["id_of_length_1_among_bare"] = record(b"@x", b"+") + record(b"@", b"+") + record(b"@yy", b"+")
    c["empty_id_bare_third"] = record(b"", b"+")
    c["empty_id_empty_third"] = record(b"", b"")
    c["empty_third"] = record(b"@id", b"")
    c["third_without_plus"] = record(b"@id 1", b"-id 1")
    c["third_of_length_1_without_plus"] = record(b"@id 1", b"-")
    c["third_of_length_1_without_plus_id_of_length_1"] = record(b"@", b"@")
    c["third_one_longer"] = record(b"@id 1", b"+id 1x")
    c["third_one_shorter"] = record(b"@id 1", b"+id ")
    c["first_byte_of_the_id_is_free"] = record(b"Xid 1", b"+id 1")
    base = b"@SRR1234567.77 77 length=100/1 and some more text"       # 49 bytes: seven lanes of a group hold a part of it
    for name, p in (("first", 0), ("second", 1), ("last", len(base) - 1)):
        t = bytearray(b"+" + base[1:])
        t[p] ^= 0x01
        c["differs_at_the_%s_byte" % name] = record(base, bytes(t))
    for name, at in (("first", 0), ("middle", 20), ("last", 40)):
        recs = same_file(41)
        recs[at] = record(sra_id(at + 1), b"+" + sra_id(at + 1)[1:-1] + b"X", seed=at)
        c["violation_in_the_%s_record" % name] = b"".join(recs)
    recs = same_file(41)
    recs[17] = record(sra_id(18), b"+", seed=17)
    c["one_bare_in_a_same_file"] = b"".join(recs)
    recs = [record(sra_id(i), b"+", seed=i) for i in range(41)]
    recs[23] = record(sra_id(23), b"+" + sra_id(23)[1:], seed=23)
    c["one_same_in_a_bare_file"] = b"".join(recs)
    c["crlf_same"] = b"".join(record(sra_id(i) + b"\r", b"+" + sra_id(i)[1:] + b"\r", nl=b"\n", seed=i) for i in range(5))
    c["crlf_bare"] = b"".join(record(sra_id(i) + b"\r", b"+\r", seed=i) for i in range(5))        # "+\r" is neither bare nor the id
    full = b"".join(same_file(5))
    c["truncated_after_line_2"] = full + b"@SRR1234567.6 6 length=100\nACGT\n"
    c["truncated_after_line_2_bare"] = b"".join(record(sra_id(i), b"+") for i in range(5)) + b"@SRR1234567.6 6 length=100\nACGT\n"
    c["truncated_in_line_3_whole"] = full + b"@SRR1234567.6 6 length=100\nACGT\n+SRR1234567.6 6 length=100"
    c["truncated_in_line_3_cut"] = full + b"@SRR1234567.6 6 length=100\nACGT\n+SRR1234"
    c["truncated_in_line_3_bare"] = b"".join(record(sra_id(i), b"+") for i in range(5)) + b"@x\nACGT\n+"
    c["truncated_after_line_1"] = full + b"@SRR1234567.6 6 length=100\n"
    c["last_quality_line_open"] = full[:-1]
    c["binary_bytes"] = record(b"@\x00\xff\x80 id", b"+\x00\xff\x80 id") + record(b"@\xfe\x01", b"+\xfe\x01")
    return c


EXPECTED = {
    "empty": "bare", "one_same": "same", "one_bare": "bare", "id_of_length_1": "bare", "id_of_length_1_among_same": "same", "id_of_length_1_among_bare": "bare",
    "empty_id_bare_third": "bare", "empty_id_empty_third": "dropped", "empty_third": "dropped", "third_without_plus": "dropped",
    "third_of_length_1_without_plus": "dropped", "third_of_length_1_without_plus_id_of_length_1": "dropped", "third_one_longer": "dropped",
    "third_one_shorter": "dropped", "first_byte_of_the_id_is_free": "same", "differs_at_the_first_byte": "dropped", "differs_at_the_second_byte": "dropped",
    "differs_at_the_last_byte": "dropped", "violation_in_the_first_record": "dropped", "violation_in_the_middle_record": "dropped",
    "violation_in_the_last_record": "dropped", "one_bare_in_a_same_file": "dropped", "one_same_in_a_bare_file": "dropped", "crlf_same": "same",
    "crlf_bare": "dropped", "truncated_after_line_2": "same", "truncated_after_line_2_bare": "bare", "truncated_in_line_3_whole": "same",
    "truncated_in_line_3_cut": "dropped", "truncated_in_line_3_bare": "bare", "truncated_after_line_1": "same", "last_quality_line_open": "same",
    "binary_bytes": "same",
}


def alignment_text(k, broken=None):
    """16 records whose id lines have length k (k = 0: empty id and empty third line); record j carries a read of j + 1 bases, so that its third line starts at
    k + j + 3 bytes behind its id line: every residue mod 16, both sides of the 8-byte lane step and of the 16-byte load.  Put at every residue mod 16 of device
    memory the id lines start at every residue too.  broken = (record, byte): that byte of that record's third line is changed"""
    rng = random.Random(100 + k)
    recs = []
    for j in range(16):
        a = b"@" + bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789.:/ ") for _ in range(k - 1)) if k else b""
        t = bytearray(b"+" + a[1:] if k else b"")
        if broken and broken[0] == j:
            t[broken[1]] ^= 0x20
        recs.append(a + b"\n" + b"A" * (j + 1) + b"\n" + bytes(t) + b"\n" + b"H" * (j + 1) + b"\n")
    return b"".join(recs)
