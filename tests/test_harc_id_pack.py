"""./harc -c -q -I and ./harc -d -q with a packed id file, without a GPU: the stage binary is replaced by a stand-in that logs how it was called.  What is
tested is the script's own work: that -I sends the finished X.id through `id_pack` and removes it only on success, with and without -Q; that -I anywhere else
is refused before anything is computed; that -d -q unpacks X.id.hi into output/.id before `fastq_out`, refuses when both files are there, accepts either form
of each side file, and calls exactly what it called before when neither -I nor an .hi file is there."""
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
quality_pack) { echo packed; cat "$2"; } > "$4";;
quality_unpack) tail -n +2 "$2" > "$4";;
id_pack) [ -z "$STUB_FAIL_ID_PACK" ] || exit 1; { echo packed ids; cat "$2"; } > "$4";;
id_unpack) tail -n +2 "$2" > "$4";;
decoder|decoder_preserve) printf 'ACGT\nTTTT\n' > $2/output/output.dna;;
fastq_out) { cat "$2"; echo ids; cat "$4"; echo quality; cat "$5"; echo "mode=$7"; } > "$6";;
*) echo "stub: unknown command $1"; exit 1;;
esac
"""
FASTQ = b"@a\nACGT\n+\nHHHH\n@b\nTTTT\n+\nIIII\n"


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _calls(log):
    return [l.split() for l in log.read_text().splitlines()]


def _setup(tmp_path, order=False):
    """the stand-in, a small archive x.harc (with read_order.bin when order) -> (environment, log)"""
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


def _compress_dir(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    env, log = _setup(d)
    os.remove(d / "x.harc")
    (d / "in.fastq").write_bytes(FASTQ)
    return d, env, log


def test_c_q_I_packs_the_finished_id_file_after_the_quality_file(tmp_path):
    for k, flags in enumerate((["-q", "-I"], ["-p", "-q", "-I"], ["-I", "-q", "-Q"], ["-p", "-q", "-Q", "-I"])):
        d, env, log = _compress_dir(tmp_path, str(k))
        r = _run(["-c", str(d / "in.fastq")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = _calls(log)
        want = ["compressfq"] + (["quality_pack"] if "-Q" in flags else []) + ["id_pack"] + (["pack_order"] if "-p" in flags else [])
        assert [c[0] for c in calls] == want, calls
        assert [c for c in calls if c[0] == "id_pack"] == [["id_pack", str(d / "in.id"), "0", str(d / "in.id.hi")]], calls
        assert (d / "in.id.hi").read_bytes() == b"packed ids\n@a\n@b\n" and not (d / "in.id").exists()
        if "-Q" in flags:
            assert (d / "in.quality.hq").exists() and not (d / "in.quality").exists()
        else:                                                      # -I alone leaves the quality values as text
            assert (d / "in.quality").read_bytes() == b"HHHH\nIIII\n" and not (d / "in.quality.hq").exists()
        assert (d / "in.harc").exists() and not (d / "output").exists()


def test_a_failed_id_pack_leaves_the_id_file_and_no_output(tmp_path):
    d, env, log = _compress_dir(tmp_path, "fail")
    r = _run(["-c", str(d / "in.fastq"), "-q", "-I"], dict(env, STUB_FAIL_ID_PACK="1"))
    assert r.returncode == 1, r.stdout[-2000:]
    assert (d / "in.id").read_bytes() == b"@a\n@b\n" and not (d / "in.id.hi").exists()
    assert not (d / "output").exists() and not (d / "in.harc").exists()


def test_I_without_q_or_with_d_is_refused_before_anything_is_computed(tmp_path):
    env, log = _setup(tmp_path)
    (tmp_path / "in.fastq").write_bytes(FASTQ)
    for flags in (["-I"], ["-p", "-I"]):
        r = _run(["-c", str(tmp_path / "in.fastq")] + flags, env)
        assert r.returncode != 0 and "-I needs -q" in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "in.harc").exists()
    (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
    (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
    for flags in (["-I"], ["-q", "-I"], ["-p", "-q", "-I", "-z"]):
        r = _run(["-d", str(tmp_path / "x.harc")] + flags, env)
        assert r.returncode != 0 and "-I goes with -c -q only" in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "x.d.fastq").exists()


def test_d_q_unpacks_a_packed_id_file_before_fastq_out(tmp_path):
    for k, (flags, dec, hq) in enumerate(((["-q"], "decoder", False), (["-p", "-q"], "decoder_preserve", True), (["-q", "-z"], "decoder", True))):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d, order=dec == "decoder_preserve")
        (d / "x.id.hi").write_bytes(b"packed ids\n@a\n@b\n")
        if hq:
            (d / "x.quality.hq").write_bytes(b"packed\nHHHH\nIIII\n")
        else:
            (d / "x.quality").write_bytes(b"HHHH\nIIII\n")
        r = _run(["-d", str(d / "x.harc")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = _calls(log)
        out = str(d / "output")
        assert [c[0] for c in calls] == [dec] + (["quality_unpack"] if hq else []) + ["id_unpack", "fastq_out"], calls
        assert calls[-2] == ["id_unpack", str(d / "x.id.hi"), "0", out + "/.id"], calls[-2]
        gz = "-z" in flags
        name = "x.d.fastq.gz" if gz else "x.d.fastq"
        quality = out + "/.quality" if hq else str(d / "x.quality")
        assert calls[-1][1:] == [out + "/output.dna", "0", out + "/.id", quality, str(d / name)] + (["bgzf"] if gz else []), calls[-1]
        assert (d / name).read_bytes() == b"ACGT\nTTTT\nids\n@a\n@b\nquality\nHHHH\nIIII\nmode=%s\n" % (b"bgzf" if gz else b"")
        assert not (d / "output").exists() and (d / "x.id.hi").exists() and not (d / "x.id").exists()


def test_d_q_with_both_id_files_is_refused_and_names_both(tmp_path):
    env, log = _setup(tmp_path)
    (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
    (tmp_path / "x.id.hi").write_bytes(b"packed ids\n@a\n@b\n")
    (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
    r = _run(["-d", str(tmp_path / "x.harc"), "-q"], env)
    assert r.returncode != 0, r.stdout[-2000:]
    assert str(tmp_path / "x.id.hi") in r.stdout and (str(tmp_path / "x.id") + " ") in r.stdout, r.stdout[-2000:]
    assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "x.d.fastq").exists()


def test_without_I_and_without_an_hi_file_the_calls_are_what_they_were(tmp_path):
    d, env, log = _compress_dir(tmp_path, "c")
    r = _run(["-c", str(d / "in.fastq"), "-p", "-q", "-Q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log) == [["compressfq", str(d), "4", str(d / "in.fastq"), "8", "0", "0", "True", "True"],
                              ["quality_pack", str(d / "in.quality"), "0", str(d / "in.quality.hq")], ["pack_order", str(d), "4"]]
    assert (d / "in.id").read_bytes() == b"@a\n@b\n" and not (d / "in.id.hi").exists()
    e = tmp_path / "d"
    e.mkdir()
    env, log = _setup(e)
    (e / "x.id").write_bytes(b"@a\n@b\n")
    (e / "x.quality").write_bytes(b"HHHH\nIIII\n")
    r = _run(["-d", str(e / "x.harc"), "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    out = str(e / "output")
    assert _calls(log) == [["decoder", str(e), "0", "1"], ["fastq_out", out + "/output.dna", "0", str(e / "x.id"), str(e / "x.quality"), str(e / "x.d.fastq")]]
    # neither form of the id file: refused before anything is unpacked
    os.remove(e / "x.id")
    os.remove(log)
    r = _run(["-d", str(e / "x.harc"), "-q"], env)
    assert r.returncode != 0 and str(e / "x.id") in r.stdout and not log.exists() and not (e / "output").exists()


def test_usage_names_the_packed_id_file():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("-I", ".id.hi", "[-I]"):
        assert word in r.stdout, word
    assert "The .id file stays text" not in r.stdout
