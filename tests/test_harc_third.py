"""./harc -d -q on an archive that records the rule of the third lines (member read.third), without a GPU: the stage binary is replaced by a stand-in that logs
how it was called.  What is tested is the script's own work: read.third read strictly, the word `third` appended to fastq_out / fastq_out_pair under `same`
(behind bgzf where -z is given), the [third] line under `dropped`, and that without the member every call is what it was."""
import io
import os
import stat
import subprocess
import tarfile

import pytest

from tests.test_harc_pair import STUB as PAIR_STUB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTQ1 = b"@a 1:N\nACGT\n+a 1:N\nHHHH\n@b 1:N\nTTTT\n+b 1:N\nIIII\n"
FASTQ2 = b"@a 2:N\nCCGT\n+a 2:N\nJJJJ\n@b 2:N\nGGTT\n+b 2:N\nKKKK\n"
IDS1 = b"@a 1:N\n@b 1:N\n"

# the stand-in of tests/test_harc_pair.py; compressfq and compressfq_pair leave read.third when STUB_THIRD names a rule, as the stage program does with -q
STUB = PAIR_STUB.replace('compressfq)\n\to=$2/output; streams $o\n', 'compressfq)\n\to=$2/output; streams $o\n\t[ -z "$STUB_THIRD" ] || printf \'HARCT1\\nthird %s\\n\' "$STUB_THIRD" > $o/read.third\n') \
                .replace("\tprintf 'HARCP1\\nrecords 2\\n' > $o/read.pair\n", "\tprintf 'HARCP1\\nrecords 2\\n' > $o/read.pair\n\t[ -z \"$STUB_THIRD\" ] || printf 'HARCT1\\nthird %s\\n' \"$STUB_THIRD\" > $o/read.third\n") \
                .replace('fastq_out) echo fastq > "$6";;', 'fastq_out) echo "fastq $7 $8" > "$6";;') \
                .replace('echo "one $8 $9 ${10}" > "$6"; echo "two $8 $9 ${10}" > "$7";;', 'echo "one $8 $9 ${10} ${11}" > "$6"; echo "two $8 $9 ${10} ${11}" > "$7";;')
assert STUB.count("read.third") == 2 and "${11}" in STUB and "fastq $7 $8" in STUB


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


def _archive(tmp_path, third, pair=False, flags=()):
    env, log = _setup(tmp_path)
    args = ["-c", str(tmp_path / "in_1.fastq"), "-p", "-q"] + (["-2", str(tmp_path / "in_2.fastq")] if pair else []) + list(flags)
    r = _run(args, dict(env, STUB_THIRD=third or ""))
    assert r.returncode == 0, r.stdout[-2000:]
    os.remove(log)
    return env, log, tmp_path / "in_1.harc"


@pytest.mark.parametrize("flags", [(), ("-S",), ("-V", "-Q", "-I")])
def test_the_member_reaches_the_archive_raw_in_every_branch(tmp_path, flags):
    env, log = _setup(tmp_path)
    if "-S" in flags:
        env.pop("HARC_AMD_STAGE3")
    r = _run(["-c", str(tmp_path / "in_1.fastq"), "-p", "-q"] + list(flags), dict(env, STUB_THIRD="same"))
    assert r.returncode == 0, r.stdout[-2000:]
    names = _names(tmp_path / "in_1.harc")
    assert "./read.third" in names and "./read.third.hs" not in names, names
    assert _member(tmp_path / "in_1.harc", "read.third") == b"HARCT1\nthird same\n"
    # the script makes no call of its own for it: the list is what it is without the member
    with_calls = [c[0] for c in _calls(log)]
    os.remove(log); os.remove(tmp_path / "in_1.harc")
    for f in ("in_1.id", "in_1.quality", "in_1.id.hi", "in_1.quality.hq"):
        if (tmp_path / f).exists():
            os.remove(tmp_path / f)
    r = _run(["-c", str(tmp_path / "in_1.fastq"), "-p", "-q"] + list(flags), env)
    assert r.returncode == 0 and [c[0] for c in _calls(log)] == with_calls
    assert "./read.third" not in _names(tmp_path / "in_1.harc")


@pytest.mark.parametrize("z", [False, True])
def test_same_appends_the_word_third_to_fastq_out(tmp_path, z):
    env, log, arc = _archive(tmp_path, "same")
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q"] + (["-z"] if z else []), env)
    assert r.returncode == 0 and "[third]" not in r.stdout, r.stdout[-2000:]
    o = str(d / "output")
    ext = ".d.fastq.gz" if z else ".d.fastq"
    assert _calls(log) == [["decoder_preserve", str(d), "0", "1", "7"],
                           ["fastq_out", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / ("in_1" + ext))] + (["bgzf"] if z else []) + ["third"]]
    assert (d / ("in_1" + ext)).read_text() == ("fastq bgzf third\n" if z else "fastq third \n")
    assert not (d / "output").exists()


@pytest.mark.parametrize("z", [False, True])
def test_same_appends_the_word_third_to_fastq_out_pair(tmp_path, z):
    env, log, arc = _archive(tmp_path, "same", pair=True)
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q"] + (["-z"] if z else []), env)
    assert r.returncode == 0, r.stdout[-2000:]
    o = str(d / "output")
    ext = ".fastq.gz" if z else ".fastq"
    assert _calls(log)[-1] == ["fastq_out_pair", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / ("in_1.d.1" + ext)), str(d / ("in_1.d.2" + ext)),
                               "2", "space"] + (["bgzf"] if z else []) + ["third"]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "fastq_out_pair"]


def test_same_with_packed_side_files(tmp_path):
    env, log, arc = _archive(tmp_path, "same", flags=("-Q", "-I"))
    d = tmp_path
    r = _run(["-d", str(arc), "-p", "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    o = str(d / "output")
    assert _calls(log)[-1] == ["fastq_out", o + "/output.dna", "0", o + "/.id", o + "/.quality", str(d / "in_1.d.fastq"), "third"]


def test_dropped_prints_the_line_and_the_calls_are_todays(tmp_path):
    env, log, arc = _archive(tmp_path, "dropped")
    d = tmp_path
    for z in (False, True):
        r = _run(["-d", str(arc), "-p", "-q"] + (["-z"] if z else []), env)
        assert r.returncode == 0, r.stdout[-2000:]
        assert "[third] the input's third lines carried text other than their ids; it was not kept" in r.stdout.splitlines()
        o = str(d / "output")
        assert _calls(log) == [["decoder_preserve", str(d), "0", "1", "7"],
                               ["fastq_out", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / ("in_1.d.fastq.gz" if z else "in_1.d.fastq"))] + (["bgzf"] if z else [])]
        os.remove(log)


def test_without_the_member_the_calls_are_todays_word_for_word(tmp_path):
    env, log, arc = _archive(tmp_path, None)
    d = tmp_path
    assert "./read.third" not in _names(arc)
    r = _run(["-d", str(arc), "-p", "-q"], env)
    assert r.returncode == 0 and "[third]" not in r.stdout, r.stdout[-2000:]
    o = str(d / "output")
    assert _calls(log) == [["decoder_preserve", str(d), "0", "1", "7"],
                           ["fastq_out", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / "in_1.d.fastq")]]
    os.remove(log)
    r = _run(["-d", str(arc), "-q", "-z"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log) == [["decoder", str(d), "0", "1"],
                           ["fastq_out", o + "/output.dna", "0", str(d / "in_1.id"), str(d / "in_1.quality"), str(d / "in_1.d.fastq.gz"), "bgzf"]]


def test_v_and_d_without_q_ignore_the_member(tmp_path):
    env, log, arc = _archive(tmp_path, "same", flags=("-V",))
    d = tmp_path
    _with_member(arc, d / "bad.harc", "read.third", b"HARCT9\nnonsense\n")       # not even looked at
    for f in ("id", "quality"):
        (d / ("bad." + f)).write_bytes((d / ("in_1." + f)).read_bytes())
    r = _run(["-d", str(d / "bad.harc"), "-p"], env)
    assert r.returncode == 0 and "read.third" not in r.stdout and "[third]" not in r.stdout, r.stdout[-2000:]
    assert (d / "bad.dna.d").exists()
    os.remove(log)
    r = _run(["-v", str(d / "bad.harc"), "-p", "-q"], env)
    assert r.returncode == 0 and "[check] reads ok, order ok, ids ok, quality ok" in r.stdout and "read.third" not in r.stdout, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check", "text_digest", "text_digest"]


@pytest.mark.parametrize("record, words", [
    (b"HARCT2\nthird same\n", "read.third: line 1 is 'HARCT2', not HARCT1"),
    (b"third same\n", "read.third: line 1 is 'third same', not HARCT1"),
    (b"HARCT1\nthird bare\n", "read.third: line 2 does not parse: 'third bare'"),
    (b"HARCT1\nthird  same\n", "read.third: line 2 does not parse: 'third  same'"),
    (b"HARCT1\nthird same\nmore\n", "read.third: line 3 does not parse: 'more'"),
    (b"HARCT1\nsame\n", "read.third: line 2 does not parse: 'same'"),
    (b"HARCT1\n", "read.third: line 2 is missing"),
    (b"", "read.third: line 1 is missing"),
])
def test_a_malformed_record_is_refused_by_its_line(tmp_path, record, words):
    env, log, arc = _archive(tmp_path, "same")
    _with_member(arc, tmp_path / "bad.harc", "read.third", record)
    for f in ("id", "quality"):
        (tmp_path / ("bad." + f)).write_bytes((tmp_path / ("in_1." + f)).read_bytes())
    for flags in (["-p", "-q"], ["-q"], ["-p", "-q", "-z"]):
        r = _run(["-d", str(tmp_path / "bad.harc")] + flags, env)
        assert r.returncode == 1 and words in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists()
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad.d") or f.startswith("bad.dna")]


def test_usage_names_the_third_lines():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("read.third", "repeats its id behind the +", "[third]"):
        assert word in r.stdout, word


def test_the_stage_program_refuses_anything_else_in_the_place_of_the_trailing_words():
    """[bgzf] [third], in that order and nothing else: status 2 before a file or a device is touched"""
    stage = os.path.join(ROOT, "harc_amd", "harc_amd_stage")
    one = [stage, "fastq_out", "no.dna", "0", "no.id", "no.quality", "no.out"]
    two = [stage, "fastq_out_pair", "no.dna", "0", "no.id", "no.quality", "no.out1", "no.out2", "2", "space"]
    for base in (one, two):
        for tail in (["gz"], ["third", "bgzf"], ["bgzf", "third", "more"], ["bgzf", "bgzf"], ["third", "third"], ["Third"]):
            r = subprocess.run(base + tail, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 2 and "only 'bgzf', 'third' or 'bgzf third' can follow" in r.stdout, (tail, r.returncode, r.stdout)
        for tail in ([], ["bgzf"], ["third"], ["bgzf", "third"]):                       # these get as far as the files, which are not there
            r = subprocess.run(base + tail, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 1 and "cannot open no.dna" in r.stdout, (tail, r.returncode, r.stdout)
