"""The match by sequence without a GPU (./harc -d -M MOTIFS [-e K]; README: "-M and what it promises"): the host twin of the kernel, plain C++ with byte comparisons,
against the plain-Python restatement of tests/match_cases.py on every case; every refusal of the list with the line it names; duplicates counted once; a motif and
its reverse complement as two motifs with the same hits; and the stage program's motifs_check, which needs no device."""
import os
import subprocess

import pytest

from tests import match_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_host_twin_equals_the_restatement(name):
    import harc_amd
    c = CASES[name]
    flags, hits, found = harc_amd.motif_flags_host(c["motifs"], mc.text_of(c["reads"]), c["L"], c["k"])
    assert flags == c["flags"], name
    assert hits == c["hits"] and found == sum(c["hits"]), name
    assert harc_amd.motifs_check_host(c["motifs"], c["k"]) == len(c["parsed"])


def test_the_random_case_selects_some_reads_and_finds_three_of_four():
    c = CASES["random_2000"]
    assert len(c["reads"]) == 2000 and c["L"] == 100 and [len(p) for p in c["parsed"]][:3] == [12, 20, 33]
    assert 0 < sum(c["flags"]) < 2000 and sum(c["hits"]) == 3 and len(c["hits"]) == 4
    assert mc.missing(c["parsed"], c["hits"]) == [c["parsed"][3]]


@pytest.mark.parametrize("index", range(len(mc.refusals())))
def test_every_refusal_of_the_list_names_its_line(index):
    import harc_amd
    text, k, line = mc.refusals()[index]
    with pytest.raises(mc.Refused) as r:
        mc.parse(text, k)
    assert r.value.line == line
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.motifs_check_host(text, k)
    assert e.value.code == -1
    if line:
        assert ("line %d:" % line) in str(e.value), str(e.value)
    else:
        assert "line " not in str(e.value), str(e.value)
    with pytest.raises(harc_amd.HarcAmdError):
        harc_amd.motif_flags_host(text, b"ACGT\n", 4, k)


def test_the_refusal_of_a_byte_names_the_byte():
    import harc_amd
    for text, byte in ((b"ACGT\nAC\rT\n", "0x0d"), (b"ACGU\n", "0x55"), (b"AC GT", "0x20"), (b"ACGT\xff", "0xff")):
        with pytest.raises(harc_amd.HarcAmdError, match="byte " + byte):
            harc_amd.motifs_check_host(text)


def test_k_above_8_is_refused():
    import harc_amd
    with pytest.raises(harc_amd.HarcAmdError, match="K = 9"):
        harc_amd.motifs_check_host(b"ACGTACGTACGTACGT\n", 9)
    assert harc_amd.motifs_check_host(b"ACGTACGTACGTACGT\n", 8) == 1


def test_duplicates_count_once_and_the_edges_of_the_limits_are_taken():
    import harc_amd
    assert harc_amd.motifs_check_host(b"ACGT\nacgt\nAcGt\n>ACGT\nACGTN\n") == 2
    assert harc_amd.motifs_check_host(b"A" * 255) == 1
    many = b"".join(b"%s\n" % mc._kmer(i) for i in range(1024))
    assert harc_amd.motifs_check_host(many + many) == 1024            # 2048 lines, 1024 distinct motifs
    flags, hits, found = harc_amd.motif_flags_host(b"ACGT\nacgt\nTTTT\n", b"CCACGTCC\nCCCCCCCC\nCAAAACCC\n", 8)
    assert (flags, hits, found) == (b"\1\0\1", b"\1\1", 2)


def test_a_motif_and_its_reverse_complement_are_two_motifs_with_the_same_hits():
    import harc_amd
    p = b"AGATCGGAAGAGC"
    reads = [b"CC" + p + b"CCCCC", b"C" * 20, b"CCCC" + mc.rc(p) + b"CCC"]
    for lst in (p + b"\n" + mc.rc(p) + b"\n", p + b"\n"):
        flags, hits, found = harc_amd.motif_flags_host(lst, mc.text_of(reads), 20)
        assert flags == b"\1\0\1" and hits == b"\1" * found and found == lst.count(b"\n")
    flags, hits, found = harc_amd.motif_flags_host(p + b"\n" + mc.rc(p) + b"\n", mc.text_of(reads[1:2]), 20)
    assert (flags, hits, found) == (b"\0", b"\0\0", 0)


def test_the_filter_of_a_fastq_text():
    fq = b"@a\nAC\n+\nII\n@b\nGT\n+b\nJJ\n@c\nTT\n+\nKK\n"
    assert mc.fastq_reads(fq) == [b"AC", b"GT", b"TT"]
    assert mc.filter_fastq(fq, b"\1\0\1") == b"@a\nAC\n+\nII\n@c\nTT\n+\nKK\n" and mc.filter_fastq(fq, b"\0\0\0") == b""


def test_motifs_check_of_the_stage_program_needs_no_device(tmp_path):
    stage = os.path.join(ROOT, "harc_amd", "harc_amd_stage")
    (tmp_path / "ok.txt").write_bytes(b">adapter\nAGATCGGAAGAGC\nagatcggaagagc\nACNNNNGT")
    r = subprocess.run([stage, "motifs_check", str(tmp_path / "ok.txt"), "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout == "2 motifs\n", (r.stdout, r.stderr)
    r = subprocess.run([stage, "motifs_check", str(tmp_path / "ok.txt"), "4"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and r.stderr.startswith("line 4: ") and "every window would match" in r.stderr, (r.stdout, r.stderr)
    (tmp_path / "cr.txt").write_bytes(b"ACGT\r\n")
    r = subprocess.run([stage, "motifs_check", str(tmp_path / "cr.txt"), "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and r.stderr == "line 1: byte 0x0d is not one of ACGTNacgtn\n", (r.stdout, r.stderr)
    for words in (["motifs_check", str(tmp_path / "ok.txt")], ["motifs_check", str(tmp_path / "ok.txt"), "9"], ["motifs_check", str(tmp_path / "ok.txt"), "x"]):
        r = subprocess.run([stage] + words, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "motifs_check needs <file> <K 0..8>" in r.stderr, (words, r.stderr)
