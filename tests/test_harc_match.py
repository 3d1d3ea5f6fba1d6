"""./harc -d -M MOTIFS [-e K] without a GPU: the stage binary is replaced by a stand-in that logs how it was called (the stand-in of tests/test_harc_select.py with
records_match added; motifs_check, which needs no device, is handed to the real stage program and not logged).  What is tested is the script's own work: every
refusal of -M and -e before anything is untarred and which of two refusals wins, the one records_match call in its place with the right words for text and packed
side files, with and without -q, the pair words and the selected count handed on to fastq_out_pair, the names of what is written, a selection of nothing and a
failing verb that leave nothing, and the usage text.  On the parent commit ./harc -M prints the usage and exits 0: every test here asserts on files and calls."""
import os
import stat
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTQ1 = b"@a 1:N\nACGT\n+\nHHHH\n@b 1:N\nTTTT\n+\nIIII\n"
FASTQ2 = b"@a 2:N\nCCGT\n+\nJJJJ\n@b 2:N\nGGTT\n+\nKKKK\n"

STUB = r"""#!/bin/bash
# stand-in for harc_amd_stage: logs its arguments, writes what the real stages would leave
set -e
[ "$1" != "motifs_check" ] || exec "$REAL_STAGE" "$@"
echo "$@" >> "$STUB_LOG"
streams()
{
	for s in read_seq read_pos read_noise read_noisepos read_rev; do echo x > $1/$s.txt.0; done
	echo x > $1/input_N.dna; echo x > $1/read_singleton.txt; echo 4 > $1/read_meta.txt; echo x > $1/read_order.bin; echo x > $1/numreads.bin
	echo x > $1/read_order_N.bin; echo x > $1/read_order_N_pe.bin
}
# lines $2 .. $2 + $3 - 1 of the file $1, counted from 0
lines() { tail -n +$(($2 + 1)) "$1" | head -n $3; }
case $1 in
compressfq)
	o=$2/output; streams $o
	printf 'HHHH\nIIII\n' > $o/output.quality; printf '@a 1:N\n@b 1:N\n' > $o/output.id
	[ -z "$STUB_THIRD" ] || printf 'HARCT1\nthird %s\n' "$STUB_THIRD" > $o/read.third
	if [ "${10}" == "check" ]; then printf 'HARCV1\nreads %s\norder %s\n' "00000000000000aa 00000000000000bb 00000000000000cc" "0000000000000010 00000000000000dd" > $o/read.check; fi;;
compressfq_pair)
	o=$2/output; streams $o
	printf 'HARCP1\nrecords 2\n' > $o/read.pair
	if [ "$9" == "True" ]; then printf 'HHHH\nIIII\nJJJJ\nKKKK\n' > $o/output.quality; printf '@a 1:N\n@b 1:N\n' > $o/output.id; printf '@a 2:N\n@b 2:N\n' > $o/output.id2; fi;;
id_mates) echo "${STUB_RULE:-space} 2";;
pack_order) ;;
text_digest) printf '%016x %016x %016x\n' $(wc -c < "$2") $(wc -l < "$2") $(cksum < "$2" | cut -d' ' -f1);;
reads_check) echo "00000000000000aa 00000000000000bb 00000000000000cc 0000000000000010 0000000000000002 00000000000000dd";;
quality_pack) { echo packed; cat "$2"; } > "$4";;
quality_unpack) tail -n +2 "$2" > "$4";;
id_pack) { echo ids; cat "$2"; } > "$4";;
id_unpack) tail -n +2 "$2" > "$4";;
decoder|decoder_preserve) printf 'ACGT\nTTTT\nCCGT\nGGTT\n' > $2/output/output.dna;;
records_match)
	# records_match <motifs> 0 <K> <dna> <out_dna> [q <ids> <quality> <out_ids> <out_quality>] [pair <records> <rule>]: the stand-in selects line 2 (of each file)
	[ "$STUB_MATCH" != "fail" ] || { echo "harc_amd_stage records_match failed (-1): match_files: the id file holds 3 lines, 4 are wanted" >&2; exit 1; }
	if [ "$STUB_MATCH" == "zero" ]; then : > "$6"; [ "$7" != "q" ] || { : > "${10}"; : > "${11}"; }; echo "[match] 2 motifs, 0 found, 0 of 2 records"; exit 0; fi
	lines "$5" 1 1 > "$6"
	if [ "$7" == "q" ]; then
		lines "$8" 1 1 > "${10}"; lines "$9" 1 1 > "${11}"
		if [ "${12}" == "pair" ]; then
			lines "$5" 3 1 >> "$6"; lines "$9" 3 1 >> "${11}"
			[ "${14}" != "none" ] || lines "$8" 3 1 >> "${10}"
		fi
	fi
	echo "[match] 2 motifs, 1 found, 1 of 2 records"; echo "[match] not found: GGGGGGGG";;
fastq_out) { echo "fastq $7 $8"; cat "$2" "$4" "$5"; } > "$6";;
fastq_out_pair) { echo "one $8 $9 ${10}"; cat "$2" "$4" "$5"; } > "$6"; echo "two $8 $9 ${10}" > "$7";;
*) echo "stub: unknown command $1"; exit 1;;
esac
"""


def _setup(tmp_path):
    stub = tmp_path / "stage_stub.sh"
    stub.write_text(STUB)
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    log = tmp_path / "stub.log"
    (tmp_path / "in_1.fastq").write_bytes(FASTQ1)
    (tmp_path / "in_2.fastq").write_bytes(FASTQ2)
    (tmp_path / "motifs.txt").write_bytes(b">t\nTTTT\nGGGGGGGG\n")
    env = dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), STUB_LOG=str(log), HARC_AMD_STAGE3="none", REAL_STAGE=os.path.join(ROOT, "harc_amd", "harc_amd_stage"))
    return env, log


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _calls(log):
    return [l.split() for l in log.read_text().splitlines()]


def _archive(tmp_path, flags=("-p", "-q"), pair=False, rule="space"):
    env, log = _setup(tmp_path)
    args = ["-c", str(tmp_path / "in_1.fastq")] + (["-2", str(tmp_path / "in_2.fastq")] if pair else []) + list(flags)
    r = _run(args, dict(env, STUB_RULE=rule))
    assert r.returncode == 0, r.stdout[-2000:]
    os.remove(log)
    return env, log, tmp_path / "in_1.harc"


def _left(d):
    """what lies next to the archive that a restore could have written"""
    return sorted(f for f in os.listdir(d) if ".d." in f or f.endswith(".dna.d") or f == "output")


# ------------------------------------------------------------------------------------------------ refusals before anything is untarred
def test_refusals_of_M_and_e_before_anything_is_untarred(tmp_path):
    env, log, arc = _archive(tmp_path)
    d = tmp_path
    motifs = str(d / "motifs.txt")
    (d / "names.txt").write_bytes(b"b\n")
    (d / "empty.txt").write_bytes(b"")
    (d / "cr.txt").write_bytes(b"ACGT\r\nTTTT\r\n")
    (d / "headers.txt").write_bytes(b">one\n\n>two\n")
    (d / "short.txt").write_bytes(b"ACGTACGT\n>x\nACNNNNGT\n")
    (d / "adir").mkdir()
    big = d / "big.txt"
    with open(big, "wb") as f:                                         # a sparse file: one byte more than a list may hold
        f.truncate(2 ** 20 + 1)
    a = str(arc)
    cases = [
        (["-c", str(d / "in_1.fastq"), "-p", "-q", "-M", motifs], "-M goes with -d only"),
        (["-v", a, "-p", "-q", "-M", motifs], "-M goes with -d only"),
        (["-R", a, "-M", motifs], "-M goes with -d only"),
        (["-d", a, "-p", "-r", "1:2", "-M", motifs], "-M does not go with -r"),
        (["-d", a, "-p", "-q", "-L", str(d / "names.txt"), "-M", motifs], "-M does not go with -L"),
        (["-d", a, "-p", "-e", "1"], "-e goes with -M only"),
        (["-c", str(d / "in_1.fastq"), "-e", "1"], "-e goes with -M only"),
        (["-d", a, "-p", "-M", motifs, "-e", "9"], "-e 9: not a number of mismatches, an integer from 0 to 8"),
        (["-d", a, "-p", "-M", motifs, "-e", "x"], "-e x: not a number of mismatches"),
        (["-d", a, "-p", "-M", motifs, "-e", "-1"], "-e -1: not a number of mismatches"),
        (["-d", a, "-p", "-M", motifs, "-e", "1.5"], "-e 1.5: not a number of mismatches"),
        (["-d", a, "-p", "-M", str(d / "missing.txt")], "-M %s: no such file" % (d / "missing.txt")),
        (["-d", a, "-p", "-q", "-M", str(d / "adir")], "-M %s: no such file, or not a regular file" % (d / "adir")),
        (["-d", a, "-p", "-q", "-z", "-M", str(d / "empty.txt")], "-M %s: the list is empty" % (d / "empty.txt")),
        (["-d", a, "-p", "-M", str(big)], "-M %s: 1048577 bytes are more than the 2^20 of a list of motifs" % big),
        (["-d", a, "-p", "-M", str(d / "cr.txt")], "-M %s: line 1: byte 0x0d is not one of ACGTNacgtn" % (d / "cr.txt")),
        (["-d", a, "-p", "-M", str(d / "headers.txt")], "-M %s: the list holds no motif" % (d / "headers.txt")),
        (["-d", a, "-p", "-q", "-M", str(d / "short.txt"), "-e", "4"], "-M %s: line 3: the motif has 4 bases that are not N" % (d / "short.txt")),
        (["-d", a, "-p", "-q", "-M", str(d / "short.txt"), "-e", "8"], "-M %s: line 1: the motif has 8 bases that are not N" % (d / "short.txt")),
        # of two refusals that apply, the first in the order of the command line's checks wins
        (["-c", str(d / "in_1.fastq"), "-r", "1:2", "-M", motifs], "-r goes with -d only"),
        (["-d", a, "-L", str(d / "names.txt"), "-M", motifs], "-L needs -q"),
        (["-v", a, "-M", motifs, "-e", "9"], "-M goes with -d only"),
        (["-d", a, "-r", "1:2", "-M", str(d / "missing.txt"), "-e", "9"], "-M does not go with -r"),
        (["-d", a, "-M", str(d / "missing.txt"), "-e", "9"], "-e 9: not a number of mismatches"),
        (["-d", a, "-M", str(d / "empty.txt"), "-z"], "-z needs -q"),
        (["-d", a, "-M", str(d / "cr.txt"), "-Q"], "-M %s: line 1" % (d / "cr.txt")),
    ]
    for args, words in cases:
        r = _run(args, env)
        assert r.returncode == 1 and r.stdout.startswith(words), (args, r.stdout[-2000:])
        assert not log.exists() and not _left(d), (args, _left(d))
    # the refusals of -d -q that stand in front of everything stay there
    os.remove(d / "in_1.id")
    r = _run(["-d", a, "-p", "-q", "-M", motifs], env)
    assert r.returncode == 1 and "-q needs" in r.stdout and "in_1.id" in r.stdout and not log.exists() and not _left(d), r.stdout[-2000:]
    (d / "in_1.id").write_bytes(b"@a 1:N\n@b 1:N\n")
    (d / "in_1.id.hi").write_bytes(b"ids\n@a 1:N\n@b 1:N\n")
    r = _run(["-d", a, "-p", "-q", "-M", motifs], env)
    assert r.returncode == 1 and "both" in r.stdout and "remove one" in r.stdout and not log.exists() and not _left(d), r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ a plain archive
@pytest.mark.parametrize("packed_quality", [False, True])
@pytest.mark.parametrize("packed_ids", [False, True])
def test_d_q_M_calls_records_match_once_in_its_place(tmp_path, packed_quality, packed_ids):
    flags = ("-p", "-q") + (("-Q",) if packed_quality else ()) + (("-I",) if packed_ids else ())
    env, log, arc = _archive(tmp_path, flags)
    d = tmp_path
    o = str(d / "output")
    motifs = str(d / "motifs.txt")
    q = o + "/.quality" if packed_quality else str(d / "in_1.quality")
    i = o + "/.id" if packed_ids else str(d / "in_1.id")
    unpack = ([["quality_unpack", str(d / "in_1.quality.hq"), "0", q]] if packed_quality else []) + ([["id_unpack", str(d / "in_1.id.hi"), "0", i]] if packed_ids else [])
    for args, k, first, name, tail in ((["-p", "-q"], "0", ["decoder_preserve", str(d), "0", "1", "7"], "in_1.hit.d.fastq", []),
                                       (["-q", "-z", "-e", "2"], "2", ["decoder", str(d), "0", "1"], "in_1.hit.d.fastq.gz", ["bgzf"])):
        r = _run(["-d", str(arc)] + args + ["-M", motifs], env)
        assert r.returncode == 0, r.stdout[-2000:]
        match = ["records_match", motifs, "0", k, o + "/output.dna", o + "/.hit.dna", "q", i, q, o + "/.hit.id", o + "/.hit.quality"]
        want = [first] + unpack + [match, ["fastq_out", o + "/.hit.dna", "0", o + "/.hit.id", o + "/.hit.quality", str(d / name)] + tail]
        assert _calls(log) == want, _calls(log)
        # the stand-in's fastq_out writes the three texts it was given: record 2 of each
        assert (d / name).read_bytes() == b"fastq %s \nTTTT\n@b 1:N\nIIII\n" % (b"bgzf" if tail else b""), (d / name).read_bytes()
        assert "[match] 2 motifs, 1 found, 1 of 2 records" in r.stdout and "[match] not found: GGGGGGGG" in r.stdout
        assert not (d / "output").exists() and not (d / "in_1.d.fastq").exists()
        os.remove(log)
    assert _left(d) == ["in_1.hit.d.fastq", "in_1.hit.d.fastq.gz"]


@pytest.mark.parametrize("pair", [False, True])
def test_d_M_without_q_filters_the_reads_alone(tmp_path, pair):
    env, log, arc = _archive(tmp_path, pair=pair)
    d = tmp_path
    o = str(d / "output")
    motifs = str(d / "motifs.txt")
    for args, first in ((["-p", "-e", "1"], ["decoder_preserve", str(d), "0", "1", "7"]), (["-e", "1"], ["decoder", str(d), "0", "1"])):
        r = _run(["-d", str(arc)] + args + ["-M", motifs], env)
        assert r.returncode == 0, r.stdout[-2000:]
        # no side file is named, and on the archive of a pair no pair words: the plain X.dna.d, filtered line by line
        assert _calls(log) == [first, ["records_match", motifs, "0", "1", o + "/output.dna", o + "/.hit.dna"]], _calls(log)
        assert (d / "in_1.hit.dna.d").read_bytes() == b"TTTT\n" and _left(d) == ["in_1.hit.dna.d"]
        os.remove(log)
        os.remove(d / "in_1.hit.dna.d")


def test_a_checked_archive_is_checked_whole_in_front_of_the_match(tmp_path):
    env, log, arc = _archive(tmp_path, ("-p", "-q", "-V"))
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q", "-M", str(d / "motifs.txt")], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check", "text_digest", "text_digest", "records_match", "fastq_out"]
    assert "[check] reads ok, order ok" in r.stdout and "not checked: -r" not in r.stdout
    assert r.stdout.index("[check]") < r.stdout.index("[match]")
    assert _left(d) == ["in_1.hit.d.fastq"]
    os.remove(log)
    os.remove(d / "in_1.hit.d.fastq")
    r = _run(["-d", str(arc), "-p", "-M", str(d / "motifs.txt")], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check", "records_match"] and r.stdout.index("[check]") < r.stdout.index("[match]")
    assert _left(d) == ["in_1.hit.dna.d"]


def test_third_lines_are_passed_on_unchanged(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(["-c", str(d / "in_1.fastq"), "-p", "-q"], dict(env, STUB_THIRD="same"))
    assert r.returncode == 0, r.stdout[-2000:]
    os.remove(log)
    o = str(d / "output")
    r = _run(["-d", str(d / "in_1.harc"), "-p", "-q", "-z", "-M", str(d / "motifs.txt")], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log)[-1] == ["fastq_out", o + "/.hit.dna", "0", o + "/.hit.id", o + "/.hit.quality", str(d / "in_1.hit.d.fastq.gz"), "bgzf", "third"]


# ------------------------------------------------------------------------------------------------ the archive of a pair
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rule", ["space", "none"])
def test_d_p_q_M_on_the_archive_of_a_pair(tmp_path, rule, packed):
    flags = ("-p", "-q") + (("-Q", "-I") if packed else ())
    env, log, arc = _archive(tmp_path, flags, pair=True, rule=rule)
    d = tmp_path
    o = str(d / "output")
    motifs = str(d / "motifs.txt")
    q = o + "/.quality" if packed else str(d / "in_1.quality")
    i = o + "/.id" if packed else str(d / "in_1.id")
    r = _run(["-d", str(arc), "-p", "-q", "-M", motifs, "-e", "3"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    calls = _calls(log)
    assert [c[0] for c in calls] == ["decoder_preserve"] + (["quality_unpack", "id_unpack"] if packed else []) + ["records_match", "fastq_out_pair"]
    assert calls[-2] == ["records_match", motifs, "0", "3", o + "/output.dna", o + "/.hit.dna", "q", i, q, o + "/.hit.id", o + "/.hit.quality", "pair", "2", rule]
    # the selected count, not the archive's, goes to fastq_out_pair
    assert calls[-1] == ["fastq_out_pair", o + "/.hit.dna", "0", o + "/.hit.id", o + "/.hit.quality", str(d / "in_1.hit.d.1.fastq"), str(d / "in_1.hit.d.2.fastq"), "1", rule]
    ids = b"@b 1:N\n@b 2:N\n" if rule == "none" else b"@b 1:N\n"
    assert (d / "in_1.hit.d.1.fastq").read_bytes() == b"one 1 %s \nTTTT\nGGTT\n%sIIII\nKKKK\n" % (rule.encode(), ids)
    assert _left(d) == ["in_1.hit.d.1.fastq", "in_1.hit.d.2.fastq"]
    os.remove(log)
    r = _run(["-d", str(arc), "-p", "-q", "-z", "-M", motifs], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log)[-1][5:] == [str(d / "in_1.hit.d.1.fastq.gz"), str(d / "in_1.hit.d.2.fastq.gz"), "1", rule, "bgzf"]


def test_a_pair_without_p_is_refused_as_before(tmp_path):
    env, log, arc = _archive(tmp_path, pair=True)
    r = _run(["-d", str(arc), "-q", "-M", str(tmp_path / "motifs.txt")], env)
    assert r.returncode == 1 and "-q needs -p on an archive of a pair" in r.stdout and not log.exists() and not _left(tmp_path), r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ nothing selected, a failing verb
@pytest.mark.parametrize("args", [["-p", "-q"], ["-p", "-q", "-z"], ["-p"], []])
@pytest.mark.parametrize("pair", [False, True])
def test_a_match_of_nothing_is_status_1_and_writes_nothing(tmp_path, pair, args):
    if pair and args == []:
        args = ["-p", "-q", "-e", "1"]
    env, log, arc = _archive(tmp_path, pair=pair)
    d = tmp_path
    r = _run(["-d", str(arc)] + args + ["-M", str(d / "motifs.txt")], dict(env, STUB_MATCH="zero"))
    assert r.returncode == 1, r.stdout[-2000:]
    assert "[match] no read of in_1 matches one of the 2 motifs" in r.stdout
    assert [c[0] for c in _calls(log)][-1] == "records_match" and not _left(d)


@pytest.mark.parametrize("args", [["-p", "-q", "-z"], ["-p"]])
def test_a_failing_verb_leaves_nothing(tmp_path, args):
    env, log, arc = _archive(tmp_path)
    d = tmp_path
    r = _run(["-d", str(arc)] + args + ["-M", str(d / "motifs.txt")], dict(env, STUB_MATCH="fail"))
    assert r.returncode == 1 and "the id file holds 3 lines, 4 are wanted" in r.stdout, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)][-1] == "records_match" and not _left(d)


def test_without_M_nothing_changes(tmp_path):
    env, log, arc = _archive(tmp_path)
    d = tmp_path
    o = str(d / "output")
    r = _run(["-d", str(arc), "-p", "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log) == [["decoder_preserve", str(d), "0", "1", "7"], ["fastq_out", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / "in_1.d.fastq")]]
    assert "[match]" not in r.stdout and _left(d) == ["in_1.d.fastq"]
    os.remove(log)
    r = _run(["-d", str(arc), "-p"], env)
    assert r.returncode == 0 and _calls(log) == [["decoder_preserve", str(d), "0", "1", "7"]], r.stdout[-2000:]
    assert (d / "in_1.dna.d").read_bytes() == b"ACGT\nTTTT\nCCGT\nGGTT\n"


def test_usage_names_the_motifs_and_the_mismatches():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("[-M MOTIFS_file [-e K]]", "-M MOTIFS_file Only with -d", "-e K Only with -M", "X.hit.dna.d", "X.hit.d.fastq", "X.hit.d.fastq.gz", "X.hit.d.1.fastq",
                 "[match] not found: <motif>", "reverse complement", "from 0 to 8"):
        assert word in r.stdout, word
