"""./harc -d -r FIRST:LAST without a GPU: the stage binary is replaced by a stand-in that logs how it was called (the stand-in of tests/test_harc_pair.py with
the commands of the range restore added).  What is tested is the script's own work: every refusal of -r before anything is untarred, the exact calls of a range
restore on a plain archive and on the archive of a pair, with each side file as text and packed, the slices it cuts itself, the names of what it writes, the
"[check] not checked" line, and the refusal of a LAST beyond what read.pair records."""
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
quality_unpack_range|id_unpack_range) tail -n +2 "$2" > "$4.all"; lines "$4.all" $5 $6 > "$4"; rm "$4.all";;
line_range) echo "$(head -n $3 "$2" | wc -c) $(head -n $(($3 + $4)) "$2" | wc -c)";;
decoder|decoder_preserve) printf 'ACGT\nTTTT\nCCGT\nGGTT\n' > $2/output/output.dna;;
decoder_range|decoder_preserve_range)
	[ -z "$STUB_FAIL_RANGE" ] || { echo "lines 1 .. 9 are wanted, the archive holds 4" >&2; exit 1; }
	printf 'TTTT\n' > $2/output/output.dna;;
fastq_out) { echo "fastq $7"; cat "$4" "$5"; } > "$6";;
fastq_out_pair) { echo "one $8 $9 ${10}"; cat "$4" "$5"; } > "$6"; echo "two $8 $9 ${10}" > "$7";;
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
    return dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), STUB_LOG=str(log), HARC_AMD_STAGE3="none"), log


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
def test_refusals_of_r_before_anything_is_untarred(tmp_path):
    env, log, arc = _archive(tmp_path)
    d = tmp_path
    cases = [
        (["-c", str(d / "in_1.fastq"), "-r", "1:2"], "-r goes with -d only"),
        (["-c", str(d / "in_1.fastq"), "-p", "-q", "-r", "1:2"], "-r goes with -d only"),
        (["-v", str(arc), "-r", "1:2"], "-r goes with -d only"),
        (["-v", str(arc), "-p", "-q", "-r", "1:2"], "-r goes with -d only"),
    ]
    for spec in ("1", "1:", ":2", "a:b", "1:2:3", "1.5:3", "1-2", "0x1:2", " 1:2", "1:2 ", "-1:4", "1:-4", "", ":"):
        cases.append((["-d", str(arc), "-r", spec], "-r %s: not a range FIRST:LAST of two decimal numbers" % spec))
        cases.append((["-d", str(arc), "-p", "-q", "-z", "-r", spec], "-r %s: not a range FIRST:LAST of two decimal numbers" % spec))
    cases += [
        (["-d", str(arc), "-r", "0:5"], "-r 0:5: FIRST is 0, lines and records are counted from 1"),
        (["-d", str(arc), "-r", "000:5"], "-r 000:5: FIRST is 0, lines and records are counted from 1"),
        (["-d", str(arc), "-q", "-r", "5:4"], "-r 5:4: LAST 4 lies in front of FIRST 5"),
        (["-d", str(arc), "-q", "-r", "010:9"], "-r 010:9: LAST 9 lies in front of FIRST 10"),      # decimal, whatever the zeros in front
    ]
    for args, words in cases:
        r = _run(args, env)
        assert r.returncode == 1 and r.stdout.startswith(words), (args, r.stdout[-2000:])
        assert not log.exists() and not _left(d), (args, _left(d))
    # the refusals of -d -q that stand in front of everything stay there
    os.remove(d / "in_1.id")
    r = _run(["-d", str(arc), "-q", "-r", "1:1"], env)
    assert r.returncode == 1 and "-q needs" in r.stdout and "in_1.id" in r.stdout and not log.exists() and not _left(d), r.stdout[-2000:]
    (d / "in_1.id").write_bytes(b"@a 1:N\n@b 1:N\n")
    (d / "in_1.id.hi").write_bytes(b"ids\n@a 1:N\n@b 1:N\n")
    r = _run(["-d", str(arc), "-q", "-r", "1:1"], env)
    assert r.returncode == 1 and "both" in r.stdout and "remove one" in r.stdout and not log.exists() and not _left(d), r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ a plain archive
def test_d_r_without_q_calls_the_range_decoder_and_names_the_slice(tmp_path):
    env, log, arc = _archive(tmp_path, ("-p",))
    d = tmp_path
    r = _run(["-d", str(arc), "-r", "2:3"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log) == [["decoder_range", str(d), "0", "1", "1", "2"]]
    assert _left(d) == ["in_1.2-3.dna.d"]
    os.remove(log)
    r = _run(["-d", str(arc), "-p", "-r", "4:4", "-m", "3"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log) == [["decoder_preserve_range", str(d), "0", "1", "3", "3", "1"]]
    assert _left(d) == ["in_1.2-3.dna.d", "in_1.4-4.dna.d"]


@pytest.mark.parametrize("packed_quality", [False, True])
@pytest.mark.parametrize("packed_ids", [False, True])
def test_d_q_r_cuts_a_slice_of_each_side_file_whatever_its_form(tmp_path, packed_quality, packed_ids):
    flags = ("-p", "-q") + (("-Q",) if packed_quality else ()) + (("-I",) if packed_ids else ())
    env, log, arc = _archive(tmp_path, flags)
    d = tmp_path
    o = str(d / "output")
    q, i = str(d / "in_1.quality"), str(d / "in_1.id")
    quality_call = ["quality_unpack_range", q + ".hq", "0", o + "/.quality.part", "1", "1"] if packed_quality else None
    id_call = ["id_unpack_range", i + ".hi", "0", o + "/.id.part", "1", "1"] if packed_ids else ["line_range", i, "1", "1"]
    for k, (args, first, name, tail) in enumerate(((["-p", "-q"], "decoder_preserve_range", "in_1.2-2.d.fastq", []), (["-q", "-z"], "decoder_range", "in_1.2-2.d.fastq.gz", ["bgzf"]))):
        r = _run(["-d", str(arc)] + args + ["-r", "2:2"], env)
        assert r.returncode == 0, r.stdout[-2000:]
        want = [[first, str(d), "0", "1"] + (["7"] if "-p" in args else []) + ["1", "1"]] + ([quality_call] if quality_call else []) + [id_call]
        want.append(["fastq_out", o + "/output.dna", "0", o + "/.id", o + "/.quality", str(d / name)] + tail)
        assert _calls(log) == want, _calls(log)
        # the stand-in's fastq_out writes the side files it was given: line 2 of each, whatever cut it
        assert (d / name).read_bytes() == b"fastq %s\n@b 1:N\nIIII\n" % (b"bgzf" if tail else b""), (d / name).read_bytes()
        assert not (d / "output").exists() and not (d / "in_1.d.fastq").exists()
        os.remove(log)
    # the whole file as a range: the same calls with 0 2, both lines
    r = _run(["-d", str(arc), "-p", "-q", "-r", "1:2"], env)
    assert r.returncode == 0 and (d / "in_1.1-2.d.fastq").read_bytes() == b"fastq \n@a 1:N\n@b 1:N\nHHHH\nIIII\n", r.stdout[-2000:]


def test_an_archive_with_a_record_says_that_a_part_is_not_checked(tmp_path):
    env, log, arc = _archive(tmp_path, ("-p", "-q", "-V"))
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q", "-r", "1:1"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "[check] not checked: -r restores a part of the archive (./harc -v checks all of it)" in r.stdout and "ok" not in r.stdout.split("[check]")[1].splitlines()[0]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve_range", "line_range", "fastq_out"]           # no reads_check, no text_digest
    assert _left(d) == ["in_1.1-1.d.fastq"]
    os.remove(log)
    # without -r the archive is checked as it was
    r = _run(["-d", str(arc), "-p", "-q"], env)
    assert r.returncode == 0 and "not checked: -r" not in r.stdout and [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check", "text_digest", "text_digest", "fastq_out"]


def test_a_range_that_the_stage_program_refuses_leaves_nothing(tmp_path):
    env, log, arc = _archive(tmp_path)
    d = tmp_path
    for args in (["-r", "1:9"], ["-p", "-q", "-r", "1:9"]):
        r = _run(["-d", str(arc)] + args, dict(env, STUB_FAIL_RANGE="1"))
        assert r.returncode == 1 and "lines 1 .. 9 are wanted, the archive holds 4" in r.stdout, r.stdout[-2000:]
        assert len(_calls(log)) == 1 and not _left(d)
        os.remove(log)


# ------------------------------------------------------------------------------------------------ the archive of a pair
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rule", ["space", "none"])
def test_d_p_q_r_on_the_archive_of_a_pair(tmp_path, rule, packed):
    flags = ("-p", "-q") + (("-Q", "-I") if packed else ())
    env, log, arc = _archive(tmp_path, flags, pair=True, rule=rule)
    d = tmp_path
    o = str(d / "output")
    q, i = str(d / "in_1.quality"), str(d / "in_1.id")
    r = _run(["-d", str(arc), "-p", "-q", "-r", "2:2"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    want = [["decoder_preserve_range", str(d), "0", "1", "7", "1", "1", "3", "1"]]                      # record 2 of file 1, record 2 of file 2
    if packed:
        want += [["quality_unpack_range", q + ".hq", "0", o + "/.quality.part", "1", "1"], ["quality_unpack_range", q + ".hq", "0", o + "/.quality.part", "3", "1"]]
        want += [["id_unpack_range", i + ".hi", "0", o + "/.id.part", "1", "1"]] + ([["id_unpack_range", i + ".hi", "0", o + "/.id.part", "3", "1"]] if rule == "none" else [])
    else:
        want += [["line_range", i, "1", "1"]] + ([["line_range", i, "3", "1"]] if rule == "none" else [])
    want.append(["fastq_out_pair", o + "/output.dna", "0", o + "/.id", o + "/.quality", str(d / "in_1.2-2.d.1.fastq"), str(d / "in_1.2-2.d.2.fastq"), "1", rule])
    assert _calls(log) == want, _calls(log)
    ids = b"@b 1:N\n@b 2:N\n" if rule == "none" else b"@b 1:N\n"          # one rule for the pair: one slice, which fastq_out_pair uses for both files
    assert (d / "in_1.2-2.d.1.fastq").read_bytes() == b"one 1 %s \n%sIIII\nKKKK\n" % (rule.encode(), ids)
    assert _left(d) == ["in_1.2-2.d.1.fastq", "in_1.2-2.d.2.fastq"]
    os.remove(log)
    r = _run(["-d", str(arc), "-p", "-q", "-z", "-r", "1:2"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log)[0] == ["decoder_preserve_range", str(d), "0", "1", "7", "0", "2", "2", "2"]
    assert _calls(log)[-1][5:] == [str(d / "in_1.1-2.d.1.fastq.gz"), str(d / "in_1.1-2.d.2.fastq.gz"), "2", rule, "bgzf"]


def test_a_last_beyond_the_records_of_a_pair_is_refused_by_the_script(tmp_path):
    env, log, arc = _archive(tmp_path, pair=True)
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q", "-r", "2:3"], env)
    assert r.returncode == 1 and "-r 2:3: LAST is 3, each file of the pair holds 2 records" in r.stdout, r.stdout[-2000:]
    assert not log.exists() and not _left(d)
    # without -q the archive of a pair is one job of 2 x records lines: one range, and the stage program knows the total
    r = _run(["-d", str(arc), "-p", "-r", "2:3"], env)
    assert r.returncode == 0 and _calls(log) == [["decoder_preserve_range", str(d), "0", "1", "7", "1", "2"]], r.stdout[-2000:]
    assert _left(d) == ["in_1.2-3.dna.d"]


def test_usage_names_the_range():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("[-r FIRST:LAST]", "-r FIRST:LAST Only with -d", "X.FIRST-LAST.dna.d", "X.FIRST-LAST.d.fastq", "X.FIRST-LAST.d.1.fastq", "counted from 1"):
        assert word in r.stdout, word
