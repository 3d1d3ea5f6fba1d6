"""./harc -c R1 -2 R2 -p and ./harc -d -p -q on a paired archive, without a GPU: the stage binary is replaced by a stand-in that logs how it was called.  What is
tested is the script's own work: the exact calls of a pair run (compressfq_pair, id_mates before any digest or packer), what becomes of output.id2 under every
answer of id_mates, every refusal of -2 before anything is computed, read.pair read strictly at -d, fastq_out_pair called with the recorded count and rule,
and that without -2 and without read.pair the calls are what they were."""
import gzip
import io
import os
import stat
import subprocess
import tarfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTQ1 = b"@a 1:N\nACGT\n+\nHHHH\n@b 1:N\nTTTT\n+\nIIII\n"
FASTQ2 = b"@a 2:N\nCCGT\n+\nJJJJ\n@b 2:N\nGGTT\n+\nKKKK\n"
IDS1, IDS2 = b"@a 1:N\n@b 1:N\n", b"@a 2:N\n@b 2:N\n"

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
case $1 in
compressfq)
	o=$2/output; streams $o
	printf 'HHHH\nIIII\n' > $o/output.quality; printf '@a 1:N\n@b 1:N\n' > $o/output.id
	if [ "${10}" == "check" ]; then printf 'HARCV1\nreads %s\norder %s\n' "00000000000000aa 00000000000000bb 00000000000000cc" "0000000000000010 00000000000000dd" > $o/read.check; fi;;
compressfq_pair)
	[ -z "$STUB_FAIL_PAIR" ] || { echo "the two files of the pair hold different numbers of records: 2, 3"; exit 1; }
	o=$2/output; streams $o
	printf 'HARCP1\nrecords 2\n' > $o/read.pair
	if [ "$9" == "True" ]; then printf 'HHHH\nIIII\nJJJJ\nKKKK\n' > $o/output.quality; printf '@a 1:N\n@b 1:N\n' > $o/output.id; printf '@a 2:N\n@b 2:N\n' > $o/output.id2; fi
	if [ "${10}" == "check" ]; then printf 'HARCV1\nreads %s\norder %s\n' "00000000000000aa 00000000000000bb 00000000000000cc" "0000000000000010 00000000000000dd" > $o/read.check; fi;;
id_mates) [ -z "$STUB_FAIL_MATES" ] || exit 1; echo "${STUB_RULE:-space} 2";;
gunzip) exit 1;;
pack_order) ;;
text_digest) printf '%016x %016x %016x\n' $(wc -c < "$2") $(wc -l < "$2") $(cksum < "$2" | cut -d' ' -f1);;
reads_check) echo "00000000000000aa 00000000000000bb 00000000000000cc 0000000000000010 0000000000000002 00000000000000dd";;
quality_pack) { echo packed; cat "$2"; } > "$4";;
quality_unpack) tail -n +2 "$2" > "$4";;
id_pack) { echo ids; cat "$2"; } > "$4";;
id_unpack) tail -n +2 "$2" > "$4";;
streams_pack) shift 2; while [ $# -gt 0 ]; do cp "$1" "$2"; shift 2; done;;
streams_unpack) shift 2; while [ $# -gt 0 ]; do cp "$1" "$2"; shift 2; done;;
decoder|decoder_preserve) printf 'ACGT\nTTTT\nCCGT\nGGTT\n' > $2/output/output.dna;;
fastq_out) echo fastq > "$6";;
fastq_out_pair) [ -z "$STUB_FAIL_OUT" ] || exit 1; echo "one $8 $9 ${10}" > "$6"; echo "two $8 $9 ${10}" > "$7";;
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


def _names(arc):
    with tarfile.open(arc) as t:
        return sorted(m.name for m in t.getmembers())


def _member(arc, name):
    with tarfile.open(arc) as t:
        return t.extractfile("./" + name).read()


def _with_member(arc, out, name, data):
    """the archive `arc` with its member `name` replaced by `data` (None: left out) -> `out`"""
    with tarfile.open(arc) as t, tarfile.open(out, "w") as o:
        for m in t.getmembers():
            if m.name == "./" + name:
                if data is None:
                    continue
                m.size = len(data)
                o.addfile(m, io.BytesIO(data))
            else:
                o.addfile(m, t.extractfile(m) if m.isfile() else None)


def _pair_args(d):
    return ["-c", str(d / "in_1.fastq"), "-2", str(d / "in_2.fastq"), "-p"]


def test_the_calls_of_a_pair_run_with_q(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(_pair_args(d) + ["-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    o = str(d / "output")
    assert _calls(log) == [["compressfq_pair", str(d), "4", str(d / "in_1.fastq"), str(d / "in_2.fastq"), "8", "0", "0", "True"],
                           ["id_mates", o + "/output.id", o + "/output.id2"], ["pack_order", str(d), "4"]]
    # the archive and the side files follow file 1; X.id is file 1's ids; the second file's ids never reach the archive
    assert (d / "in_1.id").read_bytes() == IDS1 and (d / "in_1.quality").read_bytes() == b"HHHH\nIIII\nJJJJ\nKKKK\n"
    names = _names(d / "in_1.harc")
    assert "./read.pair" in names and not [n for n in names if "id2" in n or "output.id" in n or ".input" in n], names
    assert _member(d / "in_1.harc", "read.pair") == b"HARCP1\nrecords 2\nids space\n"
    assert not (d / "output").exists()


def test_the_calls_of_a_pair_run_with_q_Q_I_S_V_put_id_mates_before_any_digest_or_packer(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    env.pop("HARC_AMD_STAGE3")                                      # -S replaces the packer of stage III
    r = _run(_pair_args(d) + ["-q", "-Q", "-I", "-S", "-V"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    q, i, o = str(d / "in_1.quality"), str(d / "in_1.id"), str(d / "output")
    calls = _calls(log)
    assert calls[0] == ["compressfq_pair", str(d), "4", str(d / "in_1.fastq"), str(d / "in_2.fastq"), "8", "0", "0", "True", "check"]
    assert calls[1:10] == [
        ["id_mates", o + "/output.id", o + "/output.id2"],
        ["text_digest", i],
        ["text_digest", q],
        ["quality_pack", q, "0", q + ".hq"],
        ["quality_unpack", q + ".hq", "0", o + "/.check.quality"],
        ["text_digest", o + "/.check.quality"],
        ["id_pack", i, "0", i + ".hi"],
        ["id_unpack", i + ".hi", "0", o + "/.check.id"],
        ["text_digest", o + "/.check.id"],
    ], calls
    assert [c[0] for c in calls[10:]] == ["pack_order", "streams_pack"], calls
    assert (d / "in_1.id.hi").read_bytes() == b"ids\n" + IDS1                # -I packs file 1's ids
    rec = _member(d / "in_1.harc", "read.check").decode().splitlines()
    assert rec[3].startswith("ids %016x %016x " % (len(IDS1), 2)), rec                 # the digest of X.id as left: the folded text
    names = _names(d / "in_1.harc")
    assert "./read.pair" in names and "./read.check" in names and "./read.pair.hs" not in names, names      # a raw member in every branch of stage III
    assert _member(d / "in_1.harc", "read.pair") == b"HARCP1\nrecords 2\nids space\n"


@pytest.mark.parametrize("rule", ["same", "slash", "space", "none"])
def test_what_becomes_of_the_second_files_ids(tmp_path, rule):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(_pair_args(d) + ["-q"], dict(env, STUB_RULE=rule))
    assert r.returncode == 0, r.stdout[-2000:]
    assert (d / "in_1.id").read_bytes() == (IDS1 + IDS2 if rule == "none" else IDS1)
    assert _member(d / "in_1.harc", "read.pair") == b"HARCP1\nrecords 2\nids %s\n" % rule.encode()
    assert not [n for n in _names(d / "in_1.harc") if "id2" in n]


def test_a_pair_run_without_q_asks_for_no_rule(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(_pair_args(d), env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["compressfq_pair", "pack_order"]
    assert _calls(log)[0][-1] == "False"
    assert _member(d / "in_1.harc", "read.pair") == b"HARCP1\nrecords 2\n"


def test_id_mates_failing_or_answering_nonsense_leaves_nothing(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    for extra in ({"STUB_FAIL_MATES": "1"}, {"STUB_RULE": "dash"}):
        r = _run(_pair_args(d) + ["-q", "-I"], dict(env, **extra))
        assert r.returncode == 1, r.stdout[-2000:]
        assert [c[0] for c in _calls(log)] == ["compressfq_pair", "id_mates"]
        assert not (d / "in_1.harc").exists() and not (d / "output").exists() and not (d / "in_1.id.hi").exists()
        os.remove(log)


def test_a_stage_program_that_refuses_the_pair_leaves_nothing(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(_pair_args(d) + ["-q"], dict(env, STUB_FAIL_PAIR="1"))
    assert r.returncode == 1 and "different numbers of records" in r.stdout, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["compressfq_pair"]
    assert not (d / "in_1.harc").exists() and not (d / "output").exists()


def test_refusals_of_2_before_anything_is_computed(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    f1, f2 = str(d / "in_1.fastq"), str(d / "in_2.fastq")
    (d / "x.harc").write_bytes(b"")
    place = "mates are paired by their place in the two files, which only -p keeps"
    cases = [
        (["-d", str(d / "x.harc"), "-2", f2], "-2 goes with -c -p only (it "),
        (["-v", str(d / "x.harc"), "-p", "-2", f2], "-2 goes with -c -p only (it "),
        (["-c", f1, "-2", f2], "-2 needs -p: " + place),
        (["-c", f1, "-2", f2, "-q"], "-2 needs -p: " + place),
        (["-c", f1, "-2", f2, "-p", "-g", "2"], "-2 does not go with -g above 1"),
        (["-c", f1, "-2", str(d / "missing.fastq"), "-p"], "-2 " + str(d / "missing.fastq") + ": no such file"),
    ]
    for args, words in cases:
        r = _run(args, env)
        assert r.returncode == 1 and r.stdout.startswith(words), (args, r.stdout[-2000:])
        assert not log.exists() and not (d / "output").exists() and not (d / "in_1.harc").exists()
    # the output/ guard stays as it is
    (d / "output").mkdir()
    r = _run(["-c", f1, "-2", f2, "-p"], env)
    assert r.returncode == 1 and "Directory named output already exists" in r.stdout and not log.exists()
    (d / "output").rmdir()
    # first reads of different length: both lengths named, nothing computed, nothing left
    (d / "short_2.fastq").write_bytes(b"@a 2:N\nCCG\n+\nJJJ\n@b 2:N\nGGT\n+\nKKK\n")
    r = _run(["-c", f1, "-2", str(d / "short_2.fastq"), "-p", "-q"], env)
    assert r.returncode == 1 and "has 4 bases" in r.stdout and "has 3" in r.stdout, r.stdout[-2000:]
    assert not log.exists() and not (d / "output").exists() and not (d / "in_1.harc").exists()


def test_each_input_is_expanded_on_its_own(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    (d / "in_2.fastq.gz").write_bytes(gzip.compress(FASTQ2))
    r = _run(["-c", str(d / "in_1.fastq"), "-2", str(d / "in_2.fastq.gz"), "-p", "-q"], dict(env, HARC_AMD_GUNZIP="1"))
    assert r.returncode == 0, r.stdout[-2000:]
    calls = _calls(log)
    o = str(d / "output")
    assert calls[0] == ["gunzip", str(d / "in_2.fastq.gz"), "0", o + "/.input2.fastq"]          # asked first; the stand-in refuses, the host's gzip does it
    assert calls[1][:6] == ["compressfq_pair", str(d), "4", str(d / "in_1.fastq"), o + "/.input2.fastq", "8"], calls[1]
    assert not [n for n in _names(d / "in_1.harc") if ".input" in n]
    # both gzipped: the archive is named after file 1 without .gz and .fastq
    e = tmp_path / "both"
    e.mkdir()
    env2, log2 = _setup(e)
    (e / "s_1.fastq.gz").write_bytes(gzip.compress(FASTQ1))
    (e / "s_2.fastq.gz").write_bytes(gzip.compress(FASTQ2))
    r = _run(["-c", str(e / "s_1.fastq.gz"), "-2", str(e / "s_2.fastq.gz"), "-p"], env2)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log2)[0][:5] == ["compressfq_pair", str(e), "4", str(e / "output/.input.fastq"), str(e / "output/.input2.fastq")]
    assert (e / "s_1.harc").exists()


def _paired_archive(tmp_path, flags=("-q",), rule="space"):
    env, log = _setup(tmp_path)
    r = _run(_pair_args(tmp_path) + list(flags), dict(env, STUB_RULE=rule))
    assert r.returncode == 0, r.stdout[-2000:]
    os.remove(log)
    return env, log, tmp_path / "in_1.harc"


def test_d_p_q_on_a_paired_archive_calls_fastq_out_pair(tmp_path):
    for k, (flags, rule, z) in enumerate(((("-q",), "space", False), (("-q", "-Q", "-I"), "slash", True), (("-q",), "none", False))):
        d = tmp_path / str(k)
        d.mkdir()
        env, log, arc = _paired_archive(d, flags, rule)
        r = _run(["-d", str(arc), "-p", "-q"] + (["-z"] if z else []), env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = _calls(log)
        o = str(d / "output")
        packed = "-I" in flags
        assert [c[0] for c in calls] == ["decoder_preserve"] + (["quality_unpack", "id_unpack"] if packed else []) + ["fastq_out_pair"], calls
        ids, quality = (o + "/.id", o + "/.quality") if packed else (str(d / "in_1.id"), str(d / "in_1.quality"))
        ext = ".fastq.gz" if z else ".fastq"
        assert calls[-1][1:] == [o + "/output.dna", "0", ids, quality, str(d / ("in_1.d.1" + ext)), str(d / ("in_1.d.2" + ext)), "2", rule] + (["bgzf"] if z else []), calls[-1]
        assert (d / ("in_1.d.1" + ext)).read_text() == "one 2 %s %s\n" % (rule, "bgzf" if z else "")
        assert (d / ("in_1.d.2" + ext)).exists() and not (d / "in_1.d.fastq").exists() and not (d / "output").exists()


def test_other_modes_on_a_paired_archive(tmp_path):
    env, log, arc = _paired_archive(tmp_path, ("-q", "-V"))
    d = tmp_path
    # -d -p without -q: X.dna.d as always, file 1's reads, then file 2's
    r = _run(["-d", str(arc), "-p"], env)
    assert r.returncode == 0 and (d / "in_1.dna.d").read_bytes() == b"ACGT\nTTTT\nCCGT\nGGTT\n", r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check"]
    os.remove(log)
    # -d without -p is unchanged
    r = _run(["-d", str(arc)], env)
    assert r.returncode == 0 and [c[0] for c in _calls(log)] == ["decoder", "reads_check"], r.stdout[-2000:]
    os.remove(log)
    # -v is unchanged: the folded ids are what was digested
    r = _run(["-v", str(arc), "-p", "-q"], env)
    assert r.returncode == 0 and "[check] reads ok, order ok, ids ok, quality ok" in r.stdout, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check", "text_digest", "text_digest"]
    assert not (d / "in_1.d.1.fastq").exists() and not (d / "output").exists()
    os.remove(log)
    # -d -q without -p: refused after untarring and before the decoder, output/ removed
    r = _run(["-d", str(arc), "-q"], env)
    assert r.returncode == 1 and r.stdout.splitlines()[-1].startswith("-q needs -p on an archive of a pair"), r.stdout[-2000:]
    assert "mates are paired by their place in the two files, which only -p keeps" in r.stdout
    assert not log.exists() and not (d / "output").exists() and not (d / "in_1.d.fastq").exists()


def test_a_failed_fastq_out_pair_and_a_record_without_ids_leave_no_output(tmp_path):
    env, log, arc = _paired_archive(tmp_path)
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q"], dict(env, STUB_FAIL_OUT="1"))
    assert r.returncode == 1 and not (d / "output").exists() and not (d / "in_1.d.1.fastq").exists() and not (d / "in_1.d.2.fastq").exists()
    os.remove(log)
    _with_member(arc, d / "noids.harc", "read.pair", b"HARCP1\nrecords 2\n")
    (d / "noids.id").write_bytes(IDS1)
    (d / "noids.quality").write_bytes(b"HHHH\nIIII\nJJJJ\nKKKK\n")
    r = _run(["-d", str(d / "noids.harc"), "-p", "-q"], env)
    assert r.returncode == 1 and "read.pair: no line 'ids'" in r.stdout, r.stdout[-2000:]
    assert not log.exists() and not (d / "output").exists() and not (d / "noids.d.1.fastq").exists()


@pytest.mark.parametrize("record, words", [
    (b"HARCP2\nrecords 2\nids space\n", "read.pair: line 1 is 'HARCP2', not HARCP1"),
    (b"HARCP1\nrecords two\n", "read.pair: line 2 does not parse: 'records two'"),
    (b"HARCP1\nrecords 2\nids dash\n", "read.pair: line 3 does not parse: 'ids dash'"),
    (b"HARCP1\nrecords 2\nids space\nmore\n", "read.pair: line 4 does not parse: 'more'"),
    (b"HARCP1\nrecords -2\n", "read.pair: line 2 does not parse"),
    (b"HARCP1\nids space\n", "read.pair: no line 'records'"),
    (b"", "read.pair: line 1 is missing"),
])
def test_a_malformed_pair_record_is_refused_by_its_line(tmp_path, record, words):
    env, log, arc = _paired_archive(tmp_path)
    _with_member(arc, tmp_path / "bad.harc", "read.pair", record)
    for flags in (["-p", "-q"], ["-p"], []):
        r = _run(["-d", str(tmp_path / "bad.harc")] + flags, env)
        if "-q" in flags and r.returncode == 1 and "-q needs" in r.stdout and "bad.id" in r.stdout:
            (tmp_path / "bad.id").write_bytes(IDS1)
            (tmp_path / "bad.quality").write_bytes(b"HHHH\nIIII\nJJJJ\nKKKK\n")
            r = _run(["-d", str(tmp_path / "bad.harc")] + flags, env)
        assert r.returncode == 1 and words in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists()


def test_usage_names_the_pair():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("-2", "[-2 FASTQ_file_2]", "read.pair", ".d.1.fastq", ".d.2.fastq", "[-k num_chains] [-g num_gpus]"):
        assert word in r.stdout, word


def test_without_2_and_without_a_pair_record_the_calls_are_what_they_were(tmp_path):
    """the call lists of tests/test_harc_id_pack.py and tests/test_harc_check.py for the same command lines"""
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(["-c", str(d / "in_1.fastq"), "-p", "-q", "-Q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log) == [["compressfq", str(d), "4", str(d / "in_1.fastq"), "8", "0", "0", "True", "True"],
                           ["quality_pack", str(d / "in_1.quality"), "0", str(d / "in_1.quality.hq")], ["pack_order", str(d), "4"]]
    names = _names(d / "in_1.harc")
    assert "./read.pair" not in names
    os.remove(log)
    (d / "in_1.quality").write_bytes(b"HHHH\nIIII\n")
    os.remove(d / "in_1.quality.hq")
    r = _run(["-d", str(d / "in_1.harc"), "-p", "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    o = str(d / "output")
    assert _calls(log) == [["decoder_preserve", str(d), "0", "1", "7"],
                           ["fastq_out", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / "in_1.d.fastq")]]
    os.remove(log)
    r = _run(["-d", str(d / "in_1.harc"), "-q", "-z"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log) == [["decoder", str(d), "0", "1"],
                           ["fastq_out", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / "in_1.d.fastq.gz"), "bgzf"]]
