"""./harc -c -V, -d and -v without a GPU: the stage binary is replaced by a stand-in that logs how it was called.  What is tested is the script's own work: that -V
anywhere but at -c on one GPU is refused before anything is computed; the exact calls of -c -q -Q -I -b SPEC -V (map, digests, pack without a spec, unpack, digest,
and only then the removals); that a packed file which does not unpack to what was packed ends the run with the text files kept and nothing else left; that -d
refuses what does not match the record, naming the item, before an output file appears; that -v writes nothing; and that without -V the calls are what they were."""
import io
import os
import stat
import subprocess
import tarfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTQ = b"@a\nACGT\n+\nHHHH\n@b\nTTTT\n+\nIIII\n"
READS, ORDER = "00000000000000aa 00000000000000bb 00000000000000cc", "0000000000000010 00000000000000dd"

STUB = r"""#!/bin/bash
# stand-in for harc_amd_stage: logs its arguments, writes what the real stages would leave
set -e
echo "$@" >> "$STUB_LOG"
case $1 in
quality_spec) exit 0;;
compressfq)
	o=$2/output
	for s in read_seq read_pos read_noise read_noisepos read_rev; do echo x > $o/$s.txt.0; done
	echo x > $o/input_N.dna; echo x > $o/read_singleton.txt; echo 4 > $o/read_meta.txt; echo x > $o/read_order.bin; echo x > $o/numreads.bin
	echo x > $o/read_order_N.bin; echo x > $o/read_order_N_pe.bin
	printf 'HHHH\nIIII\n' > $o/output.quality; printf '@a\n@b\n' > $o/output.id
	if [ "${10}" == "check" ]; then
		printf 'HARCV1\nreads %s\n' "00000000000000aa 00000000000000bb 00000000000000cc" > $o/read.check
		if [ "$8" == "True" ]; then echo "order 0000000000000010 00000000000000dd" >> $o/read.check; fi
	fi;;
pack_order) ;;
text_digest) printf '%016x %016x %016x\n' $(wc -c < "$2") $(wc -l < "$2") $(cksum < "$2" | cut -d' ' -f1);;
reads_check) echo "${STUB_READS:-00000000000000aa 00000000000000bb 00000000000000cc} 0000000000000010 0000000000000002 ${STUB_ORDER_D:-00000000000000dd}";;
quality_map) { cat "$2" | tr 'HI' 'hi'; } > "$4";;
quality_pack) { echo "packed $5"; cat "$2"; } > "$4";;
quality_unpack) tail -n +2 "$2" > "$4"; [ -z "$STUB_BAD_QUNPACK" ] || printf 'hhhh\niiij\n' > "$4";;
id_pack) { echo ids; cat "$2"; } > "$4";;
id_unpack) tail -n +2 "$2" > "$4"; [ -z "$STUB_BAD_IUNPACK" ] || printf '@b\n@a\n' > "$4";;
decoder|decoder_preserve) printf 'ACGT\nTTTT\n' > $2/output/output.dna;;
fastq_out) echo fastq > "$6";;
*) echo "stub: unknown command $1"; exit 1;;
esac
"""


def _setup(tmp_path):
    stub = tmp_path / "stage_stub.sh"
    stub.write_text(STUB)
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    log = tmp_path / "stub.log"
    (tmp_path / "in.fastq").write_bytes(FASTQ)
    return dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), STUB_LOG=str(log), HARC_AMD_STAGE3="none"), log


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _calls(log):
    return [l.split() for l in log.read_text().splitlines()]


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


def test_V_is_refused_with_d_with_v_and_with_g_above_1_before_any_stage_call(tmp_path):
    env, log = _setup(tmp_path)
    fq = str(tmp_path / "in.fastq")
    (tmp_path / "x.harc").write_bytes(b"")
    for mode in ("-d", "-v"):
        for flags in (["-V"], ["-p", "-V"], ["-q", "-V"]):
            r = _run([mode, str(tmp_path / "x.harc")] + flags, env)
            assert r.returncode == 1 and r.stdout.startswith("-V goes with -c only (it "), r.stdout[-2000:]
            assert not log.exists() and not (tmp_path / "output").exists()
    for flags in (["-V", "-g", "2"], ["-g", "3", "-p", "-V"]):
        r = _run(["-c", fq] + flags, env)
        assert r.returncode == 1 and r.stdout.startswith("-V does not go with -g above 1"), r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "in.harc").exists()
    # in the words of the other flag refusals
    assert _run(["-d", str(tmp_path / "x.harc"), "-S"], env).stdout.startswith("-S goes with -c only (it ")
    # two modes give the usage text, as -c with -d does
    for args in (["-v", str(tmp_path / "x.harc"), "-c", fq], ["-c", fq, "-v", str(tmp_path / "x.harc")], ["-d", str(tmp_path / "x.harc"), "-v", str(tmp_path / "x.harc")]):
        r, both = _run(args, env), _run(["-c", fq, "-d", str(tmp_path / "x.harc")], env)
        assert r.stdout == both.stdout and r.returncode == both.returncode and "Usage:" in r.stdout and "-v HARC_file" in r.stdout
        assert not log.exists() and not (tmp_path / "output").exists()


def test_the_calls_of_c_q_Q_I_b_V_in_order(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(["-c", str(d / "in.fastq"), "-q", "-Q", "-I", "-b", "ill8", "-V"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    q, i, o = str(d / "in.quality"), str(d / "in.id"), str(d / "output")
    calls = _calls(log)
    assert calls[0] == ["quality_spec", "ill8"]
    assert calls[1][:2] == ["compressfq", str(d)] and calls[1][-3:] == ["False", "True", "check"] and len(calls[1]) == 10, calls[1]
    assert calls[2:] == [
        ["quality_map", q, "0", q + ".tmp", "ill8"],
        ["text_digest", i],
        ["text_digest", q + ".tmp"],
        ["quality_pack", q + ".tmp", "0", q + ".hq"],              # four words: no spec, the mapped text is what is packed
        ["quality_unpack", q + ".hq", "0", o + "/.check.quality"],
        ["text_digest", o + "/.check.quality"],
        ["id_pack", i, "0", i + ".hi"],
        ["id_unpack", i + ".hi", "0", o + "/.check.id"],
        ["text_digest", o + "/.check.id"],
    ], calls
    assert (d / "in.quality.hq").read_bytes() == b"packed \nhhhh\niiii\n" and (d / "in.id.hi").read_bytes() == b"ids\n@a\n@b\n"
    for gone in ("in.quality", "in.quality.tmp", "in.id", "output"):
        assert not (d / gone).exists(), gone
    with tarfile.open(d / "in.harc") as t:
        names = sorted(m.name for m in t.getmembers())
    assert "./read.check" in names and not [n for n in names if ".check." in n], names
    rec = _member(d / "in.harc", "read.check").decode().splitlines()
    assert rec[:2] == ["HARCV1", "reads " + READS] and rec[2].startswith("ids 0000000000000006 0000000000000002 ") and rec[3].startswith("quality 000000000000000a 0000000000000002 ")
    assert len(rec) == 4


def test_without_b_and_without_Q_the_texts_stay_and_are_digested_as_they_are(tmp_path):
    for k, (flags, qbytes) in enumerate(((["-p", "-q", "-V"], b"HHHH\nIIII\n"), (["-q", "-V", "-b", "ill8"], b"hhhh\niiii\n"))):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d)
        r = _run(["-c", str(d / "in.fastq")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        names = [c[0] for c in _calls(log)]
        assert names == (["compressfq", "text_digest", "text_digest", "pack_order"] if "-p" in flags else ["quality_spec", "compressfq", "quality_map", "text_digest", "text_digest"]), names
        assert (d / "in.quality").read_bytes() == qbytes and (d / "in.id").read_bytes() == b"@a\n@b\n" and not (d / "in.quality.tmp").exists()
        assert [c for c in _calls(log) if c[0] == "text_digest"] == [["text_digest", str(d / "in.id")], ["text_digest", str(d / "in.quality")]]
        rec = _member(d / "in.harc", "read.check").decode().splitlines()
        assert [l.split()[0] for l in rec[1:]] == (["reads", "order", "ids", "quality"] if "-p" in flags else ["reads", "ids", "quality"])


def test_a_packed_file_that_does_not_unpack_to_what_was_packed_ends_the_run_and_keeps_the_texts(tmp_path):
    for k, (bad, named) in enumerate((("STUB_BAD_QUNPACK", "in.quality.hq"), ("STUB_BAD_IUNPACK", "in.id.hi"))):
        for j, spec in enumerate(([], ["-b", "ill8"])):
            d = tmp_path / ("%d%d" % (k, j))
            d.mkdir()
            env, log = _setup(d)
            r = _run(["-c", str(d / "in.fastq"), "-q", "-Q", "-I", "-V"] + spec, dict(env, **{bad: "1"}))
            assert r.returncode == 1 and "-V: " + named + " does not unpack to" in r.stdout and "packed 00000000000000" in r.stdout and "unpacked 00000000000000" in r.stdout, r.stdout[-2000:]
            assert (d / "in.quality").read_bytes() == b"HHHH\nIIII\n" and (d / "in.id").read_bytes() == b"@a\n@b\n"
            for gone in ("in.quality.hq", "in.id.hi", "in.quality.tmp", "output", "in.harc"):
                assert not (d / gone).exists(), gone
            assert "id_pack" not in [c[0] for c in _calls(log)] or bad == "STUB_BAD_IUNPACK"       # the first mismatch ends the run


def _archive(tmp_path, flags):
    env, log = _setup(tmp_path)
    r = _run(["-c", str(tmp_path / "in.fastq")] + flags, env)
    assert r.returncode == 0, r.stdout[-2000:]
    os.remove(log)
    return env, log


def _listing(d):
    return sorted((p.name, p.stat().st_size) for p in d.iterdir() if p.name != "stub.log")


def test_d_and_v_check_what_is_recorded(tmp_path):
    env, log = _archive(tmp_path, ["-p", "-q", "-V"])
    arc = str(tmp_path / "in.harc")
    before = _listing(tmp_path)
    r = _run(["-v", arc, "-p", "-q"], env)
    assert r.returncode == 0 and "[check] reads ok, order ok, ids ok, quality ok" in r.stdout.splitlines(), r.stdout[-2000:]
    assert _listing(tmp_path) == before
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check", "text_digest", "text_digest"]
    r = _run(["-v", arc], env)
    assert r.returncode == 0 and "[check] reads ok, order not checked (no -p), ids not checked (no -q), quality not checked (no -q)" in r.stdout.splitlines(), r.stdout[-2000:]
    assert _listing(tmp_path) == before
    os.remove(log)
    r = _run(["-d", arc, "-p", "-q"], env)
    assert r.returncode == 0 and "[check] reads ok, order ok, ids ok, quality ok" in r.stdout.splitlines(), r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["decoder_preserve", "reads_check", "text_digest", "text_digest", "fastq_out"]
    assert (tmp_path / "in.d.fastq").exists() and not (tmp_path / "output").exists()
    os.remove(tmp_path / "in.d.fastq")
    # the decoded reads differ, as a multiset or in their order alone
    for var, val, item, recorded in (("STUB_READS", "00000000000000aa 00000000000000bb 00000000000000cd", "reads", READS), ("STUB_ORDER_D", "00000000000000de", "order", ORDER)):
        for mode in ("-d", "-v"):
            r = _run([mode, arc, "-p", "-q"], dict(env, **{var: val}))
            last = r.stdout.splitlines()[-1]
            assert r.returncode == 1 and last.startswith("[check] %s mismatch: recorded %s, found " % (item, recorded)) and val in last, r.stdout[-2000:]
            assert _listing(tmp_path) == before
    r = _run(["-d", arc], dict(env, STUB_ORDER_D="00000000000000de"))       # without -p the order is not looked at
    assert r.returncode == 0 and (tmp_path / "in.dna.d").exists()
    os.remove(tmp_path / "in.dna.d")


def test_d_refuses_a_record_whose_quality_line_differs_and_leaves_no_fastq(tmp_path):
    env, log = _archive(tmp_path, ["-p", "-q", "-V"])
    rec = _member(tmp_path / "in.harc", "read.check").decode().splitlines()
    assert rec[4].startswith("quality ")
    f = rec[4].split()
    f[3] = "%016x" % (int(f[3], 16) ^ 1)
    rec[4] = " ".join(f)
    _with_member(tmp_path / "in.harc", tmp_path / "bad.harc", "read.check", ("\n".join(rec) + "\n").encode())
    for name in ("id", "quality"):
        os.rename(tmp_path / ("in." + name), tmp_path / ("bad." + name))
    for mode in ("-d", "-v"):
        r = _run([mode, str(tmp_path / "bad.harc"), "-p", "-q"], env)
        assert r.returncode == 1 and r.stdout.splitlines()[-1].startswith("[check] quality mismatch: recorded " + " ".join(f[1:]) + ", found "), r.stdout[-2000:]
        assert not (tmp_path / "bad.d.fastq").exists() and not (tmp_path / "output").exists()
        assert "fastq_out" not in [c[0] for c in _calls(log)]
    r = _run(["-d", str(tmp_path / "bad.harc"), "-p"], env)         # without -q the side files are not looked at
    assert r.returncode == 0 and "quality not checked (no -q)" in r.stdout and (tmp_path / "bad.dna.d").exists()


def test_a_record_that_does_not_parse_is_refused_naming_the_line(tmp_path):
    env, log = _archive(tmp_path, ["-V"])
    good = "HARCV1\nreads " + READS + "\n"
    for k, (data, named) in enumerate(((b"HARCV2\nreads " + READS.encode() + b"\n", "read.check: line 1 is 'HARCV2', not HARCV1"),
                                      (good.encode() + b"sizes 0000000000000001\n", "read.check: line 3 does not parse: 'sizes 0000000000000001'"),
                                      (b"HARCV1\nreads 00000000000000aa 00000000000000bb\n", "read.check: line 2 does not parse"),
                                      (b"HARCV1\nreads 00000000000000AA 00000000000000bb 00000000000000cc\n", "read.check: line 2 does not parse"),
                                      (b"HARCV1\n", "read.check: no line 'reads'"), (b"", "read.check: line 1 is missing"))):
        arc = tmp_path / ("bad%d.harc" % k)
        _with_member(tmp_path / "in.harc", arc, "read.check", data)
        for mode in ("-d", "-v"):
            r = _run([mode, str(arc)], env)
            assert r.returncode == 1 and named in r.stdout, (data, r.stdout[-2000:])
            assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / ("bad%d.dna.d" % k)).exists()


def test_v_on_an_archive_without_the_member_gives_status_1_and_d_is_what_it_was(tmp_path):
    env, log = _archive(tmp_path, ["-q"])
    with tarfile.open(tmp_path / "in.harc") as t:
        assert "./read.check" not in [m.name for m in t.getmembers()]
    before = _listing(tmp_path)
    r = _run(["-v", str(tmp_path / "in.harc"), "-q"], env)
    assert r.returncode == 1 and "was not compressed with -V" in r.stdout, r.stdout[-2000:]
    assert not log.exists() and _listing(tmp_path) == before
    r = _run(["-d", str(tmp_path / "in.harc"), "-q"], env)
    assert r.returncode == 0 and "[check]" not in r.stdout, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["decoder", "fastq_out"]


def test_without_V_the_calls_are_what_they_were(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(["-c", str(d / "in.fastq"), "-q", "-Q", "-I"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    calls = _calls(log)
    assert calls[0][:2] == ["compressfq", str(d)] and calls[0][-2:] == ["False", "True"] and len(calls[0]) == 9, calls[0]      # no tenth word, not even an empty one
    assert calls[1:] == [["quality_pack", str(d / "in.quality"), "0", str(d / "in.quality.hq")], ["id_pack", str(d / "in.id"), "0", str(d / "in.id.hi")]], calls
    with tarfile.open(d / "in.harc") as t:
        assert "./read.check" not in [m.name for m in t.getmembers()]


def test_usage_names_V_and_v():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("[-V]", "-V Only with -c", "read.check", "./harc -v HARC_file [-p] [-q]", "not cryptographic", "[check] reads ok, order ok, ids ok, quality ok"):
        assert word in r.stdout, word
