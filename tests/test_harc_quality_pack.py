"""./harc -c -q -Q and ./harc -d -q with a packed quality file, without a GPU: the stage binary is replaced by a stand-in that logs how it was called.  What is
tested is the script's own work: that -Q sends the finished X.quality through `quality_pack` and removes it only on success; that -Q anywhere else is refused
before anything is computed; that -d -q unpacks X.quality.hq into output/.quality before `fastq_out`, refuses when both files are there, and calls exactly what
it called before when only X.quality is; and that the usage text names it."""
import os
import stat
import subprocess
import tarfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = r"""#!/bin/bash
# stand-in for harc_amd_stage: logs its arguments, writes what the real stages would leave
set -e
echo "$@" >> "$STUB_LOG"
case $1 in
compressfq)
	o=$2/output
	for s in read_seq read_pos read_noise read_noisepos read_rev; do echo x > $o/$s.txt.0; done
	echo x > $o/input_N.dna; echo x > $o/read_singleton.txt; echo 4 > $o/read_meta.txt; echo x > $o/read_order.bin; echo x > $o/numreads.bin
	printf 'HHHH\nIIII\n' > $o/output.quality; printf '@a\n@b\n' > $o/output.id;;
pack_order) ;;
quality_pack) [ -z "$STUB_FAIL_PACK" ] || exit 1; { echo packed; cat "$2"; } > "$4";;
quality_unpack) tail -n +2 "$2" > "$4";;
decoder|decoder_preserve) printf 'ACGT\nTTTT\n' > $2/output/output.dna;;
fastq_out) { cat "$2"; echo ids; cat "$4"; echo quality; cat "$5"; echo "mode=$7"; } > "$6";;
*) echo "stub: unknown command $1"; exit 1;;
esac
"""


def _setup(tmp_path, order=False):
    stub = tmp_path / "stage_stub.sh"
    stub.write_text(STUB)
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    src = tmp_path / "src"
    src.mkdir()
    with tarfile.open(tmp_path / "x.harc", "w") as arc:
        for s in ["read_pos", "read_noisepos", "read_noise", "read_rev", "read_seq"]:
            (src / (s + ".txt.0")).write_bytes(b"x")
            with tarfile.open(src / (s + ".tar"), "w") as tf:
                tf.add(src / (s + ".txt.0"), arcname=s + ".txt.0")
            arc.add(src / (s + ".tar"), arcname=s + ".tar")
        if order:
            (src / "read_order.bin").write_bytes(b"\0" * 8)
            arc.add(src / "read_order.bin", arcname="read_order.bin")
    log = tmp_path / "stub.log"
    env = dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), STUB_LOG=str(log), HARC_AMD_STAGE3="none")
    return env, log


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _calls(log):
    return [l.split() for l in log.read_text().splitlines()]


def test_c_q_Q_packs_the_finished_quality_file_and_removes_it_only_on_success(tmp_path):
    for k, flags in enumerate((["-q", "-Q"], ["-p", "-q", "-Q"], ["-Q", "-q"])):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d)
        os.remove(d / "x.harc")
        (d / "in.fastq").write_bytes(b"@a\nACGT\n+\nHHHH\n@b\nTTTT\n+\nIIII\n")
        r = _run(["-c", str(d / "in.fastq")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        packs = [c for c in _calls(log) if c[0] == "quality_pack"]
        assert packs == [["quality_pack", str(d / "in.quality"), "0", str(d / "in.quality.hq")]], _calls(log)
        assert [c[0] for c in _calls(log)][0] == "compressfq"
        assert (d / "in.quality.hq").read_bytes() == b"packed\nHHHH\nIIII\n" and not (d / "in.quality").exists()
        assert (d / "in.id").read_bytes() == b"@a\n@b\n" and (d / "in.harc").exists() and not (d / "output").exists()
    # a failed pack: status 1, output/ gone, X.quality stays, no archive
    d = tmp_path / "fail"
    d.mkdir()
    env, log = _setup(d)
    os.remove(d / "x.harc")
    (d / "in.fastq").write_bytes(b"@a\nACGT\n+\nHHHH\n@b\nTTTT\n+\nIIII\n")
    r = _run(["-c", str(d / "in.fastq"), "-q", "-Q"], dict(env, STUB_FAIL_PACK="1"))
    assert r.returncode == 1, r.stdout[-2000:]
    assert (d / "in.quality").read_bytes() == b"HHHH\nIIII\n" and not (d / "in.quality.hq").exists()
    assert not (d / "output").exists() and not (d / "in.harc").exists()
    # without -Q nothing is packed
    d = tmp_path / "plain"
    d.mkdir()
    env, log = _setup(d)
    os.remove(d / "x.harc")
    (d / "in.fastq").write_bytes(b"@a\nACGT\n+\nHHHH\n@b\nTTTT\n+\nIIII\n")
    r = _run(["-c", str(d / "in.fastq"), "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["compressfq"] and (d / "in.quality").exists() and not (d / "in.quality.hq").exists()


def test_Q_without_q_or_with_d_is_refused_before_anything_is_computed(tmp_path):
    env, log = _setup(tmp_path)
    (tmp_path / "in.fastq").write_bytes(b"@a\nACGT\n+\nHHHH\n")
    for flags in (["-Q"], ["-p", "-Q"]):
        r = _run(["-c", str(tmp_path / "in.fastq")] + flags, env)
        assert r.returncode != 0 and "-Q" in r.stdout and "-q" in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "in.harc").exists()
    (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
    (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
    for flags in (["-Q"], ["-q", "-Q"], ["-p", "-q", "-Q", "-z"]):
        r = _run(["-d", str(tmp_path / "x.harc")] + flags, env)
        assert r.returncode != 0 and "-Q" in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "x.d.fastq").exists()


def test_d_q_unpacks_a_packed_quality_file_before_fastq_out(tmp_path):
    for k, (flags, dec) in enumerate(((["-q"], "decoder"), (["-p", "-q"], "decoder_preserve"), (["-q", "-z"], "decoder"))):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d, order=dec == "decoder_preserve")
        (d / "x.id").write_bytes(b"@a\n@b\n")
        (d / "x.quality.hq").write_bytes(b"packed\nHHHH\nIIII\n")
        r = _run(["-d", str(d / "x.harc")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = _calls(log)
        out = str(d / "output")
        assert [c[0] for c in calls] == [dec, "quality_unpack", "fastq_out"], calls
        assert calls[1] == ["quality_unpack", str(d / "x.quality.hq"), "0", out + "/.quality"], calls[1]
        gz = "-z" in flags
        name = "x.d.fastq.gz" if gz else "x.d.fastq"
        assert calls[2][1:] == [out + "/output.dna", "0", str(d / "x.id"), out + "/.quality", str(d / name)] + (["bgzf"] if gz else []), calls[2]
        assert (d / name).read_bytes() == b"ACGT\nTTTT\nids\n@a\n@b\nquality\nHHHH\nIIII\nmode=%s\n" % (b"bgzf" if gz else b"")
        assert not (d / "output").exists() and (d / "x.quality.hq").exists() and not (d / "x.quality").exists()


def test_d_q_with_both_quality_files_is_refused_and_names_both(tmp_path):
    env, log = _setup(tmp_path)
    (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
    (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
    (tmp_path / "x.quality.hq").write_bytes(b"packed\nHHHH\nIIII\n")
    r = _run(["-d", str(tmp_path / "x.harc"), "-q"], env)
    assert r.returncode != 0, r.stdout[-2000:]
    assert str(tmp_path / "x.quality.hq") in r.stdout and (str(tmp_path / "x.quality") + " ") in r.stdout, r.stdout[-2000:]
    assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "x.d.fastq").exists()


def test_d_q_with_the_plain_quality_file_calls_what_it_always_called(tmp_path):
    env, log = _setup(tmp_path)
    (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
    (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
    r = _run(["-d", str(tmp_path / "x.harc"), "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    out = str(tmp_path / "output")
    assert _calls(log) == [["decoder", str(tmp_path), "0", "1"],
                           ["fastq_out", out + "/output.dna", "0", str(tmp_path / "x.id"), str(tmp_path / "x.quality"), str(tmp_path / "x.d.fastq")]]
    # neither file: refused as before, before anything is unpacked
    os.remove(tmp_path / "x.quality")
    os.remove(log)
    r = _run(["-d", str(tmp_path / "x.harc"), "-q"], env)
    assert r.returncode != 0 and str(tmp_path / "x.quality") in r.stdout and not log.exists() and not (tmp_path / "output").exists()


def test_usage_names_the_packed_quality_file():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("-Q", ".quality.hq", "[-q [-Q]]", "rANS"):
        assert word in r.stdout, word
