"""./harc -d -q -L NAMES without a GPU: the stage binary is replaced by a stand-in that logs how it was called (the stand-in of tests/test_harc_range.py with
records_select added).  What is tested is the script's own work: every refusal of -L before anything is untarred, the one records_select call in its place with the
right files for text and packed side files, the pair words and the selected count handed on to fastq_out_pair, the names of what is written, plain and with -z,
a selection of nothing and a failing verb that leave nothing, and the usage text."""
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
records_select)
	# records_select <names> 0 <ids> <dna> <quality> <out_ids> <out_dna> <out_quality> [pair <records> <rule>]: the stand-in selects record 2 (of each file)
	[ "$STUB_SELECT" != "fail" ] || { echo "harc_amd_stage records_select failed (2): the id file holds 3 lines, the reads 4" >&2; exit 1; }
	if [ "$STUB_SELECT" == "zero" ]; then : > "$7"; : > "$8"; : > "$9"; echo "[select] 2 names, 0 found, 0 of 2 records"; exit 0; fi
	lines "$4" 1 1 > "$7"; lines "$5" 1 1 > "$8"; lines "$6" 1 1 > "$9"
	if [ "${10}" == "pair" ]; then
		lines "$5" 3 1 >> "$8"; lines "$6" 3 1 >> "$9"
		[ "${12}" != "none" ] || lines "$4" 3 1 >> "$7"
	fi
	echo "[select] 2 names, 1 found, 1 of 2 records"; echo "[select] not found: nobody";;
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
    (tmp_path / "names.txt").write_bytes(b"b\nnobody\n")
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
def test_refusals_of_L_before_anything_is_untarred(tmp_path):
    env, log, arc = _archive(tmp_path)
    d = tmp_path
    names = str(d / "names.txt")
    (d / "empty.txt").write_bytes(b"")
    (d / "nameless.txt").write_bytes(b"\n@\n \n@ comment\n\tx\n@\ty\n")
    (d / "adir").mkdir()
    big = d / "big.txt"
    with open(big, "wb") as f:                                         # a sparse file: one byte more than a list may hold
        f.truncate(2 ** 30 + 1)
    cases = [
        (["-c", str(d / "in_1.fastq"), "-p", "-q", "-L", names], "-L goes with -d -q only"),
        (["-v", str(arc), "-p", "-q", "-L", names], "-L goes with -d -q only"),
        (["-R", str(arc), "-L", names], "-L goes with -d -q only"),
        (["-d", str(arc), "-L", names], "-L needs -q"),
        (["-d", str(arc), "-p", "-L", names], "-L needs -q"),
        (["-d", str(arc), "-p", "-q", "-r", "1:2", "-L", names], "-L does not go with -r"),
        (["-d", str(arc), "-p", "-q", "-L", str(d / "missing.txt")], "-L %s: no such file" % (d / "missing.txt")),
        (["-d", str(arc), "-p", "-q", "-L", str(d / "adir")], "-L %s: no such file, or not a regular file" % (d / "adir")),
        (["-d", str(arc), "-p", "-q", "-L", str(big)], "-L %s: 1073741825 bytes are more than the 2^30 of a list" % big),
        (["-d", str(arc), "-p", "-q", "-L", str(d / "empty.txt")], "-L %s: the list is empty" % (d / "empty.txt")),
        (["-d", str(arc), "-p", "-q", "-z", "-L", str(d / "nameless.txt")], "-L %s: no line of the list has a name" % (d / "nameless.txt")),
    ]
    for args, words in cases:
        r = _run(args, env)
        assert r.returncode == 1 and r.stdout.startswith(words), (args, r.stdout[-2000:])
        assert not log.exists() and not _left(d), (args, _left(d))
    # the refusals of -d -q that stand in front of everything stay there
    os.remove(d / "in_1.id")
    r = _run(["-d", str(arc), "-p", "-q", "-L", names], env)
    assert r.returncode == 1 and "-q needs" in r.stdout and "in_1.id" in r.stdout and not log.exists() and not _left(d), r.stdout[-2000:]
    (d / "in_1.id").write_bytes(b"@a 1:N\n@b 1:N\n")
    (d / "in_1.id.hi").write_bytes(b"ids\n@a 1:N\n@b 1:N\n")
    r = _run(["-d", str(arc), "-p", "-q", "-L", names], env)
    assert r.returncode == 1 and "both" in r.stdout and "remove one" in r.stdout and not log.exists() and not _left(d), r.stdout[-2000:]


def test_a_list_with_one_name_among_nameless_lines_is_taken(tmp_path):
    env, log, arc = _archive(tmp_path)
    (tmp_path / "names.txt").write_bytes(b"\n@\n @x\n@b/1 comment")          # the last line has a name, and no newline
    r = _run(["-d", str(arc), "-p", "-q", "-L", str(tmp_path / "names.txt")], env)
    assert r.returncode == 0 and "records_select" in [c[0] for c in _calls(log)], r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ a plain archive
@pytest.mark.parametrize("packed_quality", [False, True])
@pytest.mark.parametrize("packed_ids", [False, True])
def test_d_q_L_calls_records_select_once_in_its_place(tmp_path, packed_quality, packed_ids):
    flags = ("-p", "-q") + (("-Q",) if packed_quality else ()) + (("-I",) if packed_ids else ())
    env, log, arc = _archive(tmp_path, flags)
    d = tmp_path
    o = str(d / "output")
    names = str(d / "names.txt")
    q = o + "/.quality" if packed_quality else str(d / "in_1.quality")
    i = o + "/.id" if packed_ids else str(d / "in_1.id")
    unpack = ([["quality_unpack", str(d / "in_1.quality.hq"), "0", q]] if packed_quality else []) + ([["id_unpack", str(d / "in_1.id.hi"), "0", i]] if packed_ids else [])
    select = ["records_select", names, "0", i, o + "/output.dna", q, o + "/.sel.id", o + "/.sel.dna", o + "/.sel.quality"]
    for args, first, name, tail in ((["-p", "-q"], ["decoder_preserve", str(d), "0", "1", "7"], "in_1.sel.d.fastq", []), (["-q", "-z"], ["decoder", str(d), "0", "1"], "in_1.sel.d.fastq.gz", ["bgzf"])):
        r = _run(["-d", str(arc)] + args + ["-L", names], env)
        assert r.returncode == 0, r.stdout[-2000:]
        want = [first] + unpack + [select, ["fastq_out", o + "/.sel.dna", "0", o + "/.sel.id", o + "/.sel.quality", str(d / name)] + tail]
        assert _calls(log) == want, _calls(log)
        # the stand-in's fastq_out writes the three texts it was given: record 2 of each
        assert (d / name).read_bytes() == b"fastq %s \nTTTT\n@b 1:N\nIIII\n" % (b"bgzf" if tail else b""), (d / name).read_bytes()
        assert "[select] 2 names, 1 found, 1 of 2 records" in r.stdout and "[select] not found: nobody" in r.stdout
        assert not (d / "output").exists() and not (d / "in_1.d.fastq").exists()
        os.remove(log)
    assert _left(d) == ["in_1.sel.d.fastq", "in_1.sel.d.fastq.gz"]


def test_a_checked_archive_is_checked_whole_in_front_of_the_selection(tmp_path):
    env, log, arc = _archive(tmp_path, ("-p", "-q", "-V"))
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q", "-L", str(d / "names.txt")], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check", "text_digest", "text_digest", "records_select", "fastq_out"]
    assert "[check] reads ok, order ok" in r.stdout and "not checked: -r" not in r.stdout
    assert r.stdout.index("[check]") < r.stdout.index("[select]")
    assert _left(d) == ["in_1.sel.d.fastq"]


def test_third_lines_are_passed_on_unchanged(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(["-c", str(d / "in_1.fastq"), "-p", "-q"], dict(env, STUB_THIRD="same"))
    assert r.returncode == 0, r.stdout[-2000:]
    os.remove(log)
    o = str(d / "output")
    r = _run(["-d", str(d / "in_1.harc"), "-p", "-q", "-z", "-L", str(d / "names.txt")], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log)[-1] == ["fastq_out", o + "/.sel.dna", "0", o + "/.sel.id", o + "/.sel.quality", str(d / "in_1.sel.d.fastq.gz"), "bgzf", "third"]


# ------------------------------------------------------------------------------------------------ the archive of a pair
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rule", ["space", "none"])
def test_d_p_q_L_on_the_archive_of_a_pair(tmp_path, rule, packed):
    flags = ("-p", "-q") + (("-Q", "-I") if packed else ())
    env, log, arc = _archive(tmp_path, flags, pair=True, rule=rule)
    d = tmp_path
    o = str(d / "output")
    names = str(d / "names.txt")
    q = o + "/.quality" if packed else str(d / "in_1.quality")
    i = o + "/.id" if packed else str(d / "in_1.id")
    r = _run(["-d", str(arc), "-p", "-q", "-L", names], env)
    assert r.returncode == 0, r.stdout[-2000:]
    calls = _calls(log)
    assert [c[0] for c in calls] == ["decoder_preserve"] + (["quality_unpack", "id_unpack"] if packed else []) + ["records_select", "fastq_out_pair"]
    assert calls[-2] == ["records_select", names, "0", i, o + "/output.dna", q, o + "/.sel.id", o + "/.sel.dna", o + "/.sel.quality", "pair", "2", rule]
    # the selected count, not the archive's, goes to fastq_out_pair
    assert calls[-1] == ["fastq_out_pair", o + "/.sel.dna", "0", o + "/.sel.id", o + "/.sel.quality", str(d / "in_1.sel.d.1.fastq"), str(d / "in_1.sel.d.2.fastq"), "1", rule]
    ids = b"@b 1:N\n@b 2:N\n" if rule == "none" else b"@b 1:N\n"
    assert (d / "in_1.sel.d.1.fastq").read_bytes() == b"one 1 %s \nTTTT\nGGTT\n%sIIII\nKKKK\n" % (rule.encode(), ids)
    assert _left(d) == ["in_1.sel.d.1.fastq", "in_1.sel.d.2.fastq"]
    os.remove(log)
    r = _run(["-d", str(arc), "-p", "-q", "-z", "-L", names], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log)[-1][5:] == [str(d / "in_1.sel.d.1.fastq.gz"), str(d / "in_1.sel.d.2.fastq.gz"), "1", rule, "bgzf"]


def test_a_pair_without_p_is_refused_as_before(tmp_path):
    env, log, arc = _archive(tmp_path, pair=True)
    r = _run(["-d", str(arc), "-q", "-L", str(tmp_path / "names.txt")], env)
    assert r.returncode == 1 and "-q needs -p on an archive of a pair" in r.stdout and not log.exists() and not _left(tmp_path), r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------ nothing selected, a failing verb
@pytest.mark.parametrize("pair", [False, True])
def test_a_selection_of_nothing_is_status_1_and_writes_nothing(tmp_path, pair):
    env, log, arc = _archive(tmp_path, pair=pair)
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q", "-L", str(d / "names.txt")], dict(env, STUB_SELECT="zero"))
    assert r.returncode == 1, r.stdout[-2000:]
    assert "[select] no record of in_1 carries one of the 2 names" in r.stdout
    assert [c[0] for c in _calls(log)][-1] == "records_select" and not _left(d)


def test_a_failing_verb_leaves_nothing(tmp_path):
    env, log, arc = _archive(tmp_path)
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q", "-z", "-L", str(d / "names.txt")], dict(env, STUB_SELECT="fail"))
    assert r.returncode == 1 and "the id file holds 3 lines, the reads 4" in r.stdout, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)][-1] == "records_select" and not _left(d)


def test_without_L_nothing_changes(tmp_path):
    env, log, arc = _archive(tmp_path)
    d = tmp_path
    o = str(d / "output")
    r = _run(["-d", str(arc), "-p", "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log) == [["decoder_preserve", str(d), "0", "1", "7"], ["fastq_out", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / "in_1.d.fastq")]]
    assert "[select]" not in r.stdout and _left(d) == ["in_1.d.fastq"]


def test_usage_names_the_list():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("[-L NAMES_file]", "-L NAMES_file Only with -d -q", "X.sel.d.fastq", "X.sel.d.fastq.gz", "X.sel.d.1.fastq", "[select] not found: <name>", "/1 or /2"):
        assert word in r.stdout, word
