"""./harc -d -q without a GPU: the stage binary is replaced by a stand-in that logs how it was called, so that what is tested is the script's own
work -- that the .id and .quality files next to the archive are asked for before anything is decoded, and that the decoder's output goes through
`fastq_out` with the five paths in order and ends up as X.d.fastq."""
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
decoder|decoder_preserve) printf 'ACGT\nTTTT\n' > $2/output/output.dna;;
fastq_out) { cat "$2"; echo ids; cat "$4"; echo quality; cat "$5"; } > "$6";;
*) echo "stub: unknown command $1"; exit 1;;
esac
"""


def _setup(tmp_path):
    stub = tmp_path / "stage_stub.sh"
    stub.write_text(STUB)
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    src = tmp_path / "src"
    src.mkdir()
    for s in ["read_pos", "read_noisepos", "read_noise", "read_rev", "read_seq"]:
        (src / (s + ".txt.0")).write_bytes(b"x")
        with tarfile.open(src / (s + ".tar"), "w") as tf:
            tf.add(src / (s + ".txt.0"), arcname=s + ".txt.0")
        (src / (s + ".txt.0")).unlink()
    with tarfile.open(tmp_path / "x.harc", "w") as tf:
        for f in sorted(os.listdir(src)):
            tf.add(src / f, arcname=f)
    log = tmp_path / "stub.log"
    env = dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), STUB_LOG=str(log))
    return env, log


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_d_q_without_quality_file_is_refused_before_the_decoder_runs(tmp_path):
    env, log = _setup(tmp_path)
    (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
    r = _run(["-d", str(tmp_path / "x.harc"), "-q"], env)
    assert r.returncode != 0, r.stdout[-2000:]
    assert str(tmp_path / "x.quality") in r.stdout, r.stdout[-2000:]
    assert not (tmp_path / "output").exists()
    assert not log.exists(), log.read_text()                     # no stage was started: the decoder least of all
    assert not (tmp_path / "x.d.fastq").exists() and not (tmp_path / "x.dna.d").exists()
    # the same for the id file
    (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
    (tmp_path / "x.id").unlink()
    r = _run(["-d", str(tmp_path / "x.harc"), "-q", "-p"], env)
    assert r.returncode != 0 and str(tmp_path / "x.id") in r.stdout, r.stdout[-2000:]
    assert not (tmp_path / "output").exists() and not log.exists()


def test_d_q_runs_the_decoder_and_then_fastq_out_with_the_five_paths(tmp_path):
    for flags, dec in ([], "decoder"), (["-p"], "decoder_preserve"):
        env, log = _setup(tmp_path)
        (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
        (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
        if dec == "decoder_preserve":
            # -d -p asks for the order file of a -p archive
            with tarfile.open(tmp_path / "x.harc", "a") as tf:
                (tmp_path / "read_order.bin").write_bytes(b"\0" * 8)
                tf.add(tmp_path / "read_order.bin", arcname="read_order.bin")
        r = _run(["-d", str(tmp_path / "x.harc"), "-q"] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = [l.split() for l in log.read_text().splitlines()]
        assert [c[0] for c in calls] == [dec, "fastq_out"], calls
        out = str(tmp_path / "output")
        assert calls[1][1:] == [out + "/output.dna", "0", str(tmp_path / "x.id"), str(tmp_path / "x.quality"), str(tmp_path / "x.d.fastq")], calls[1]
        assert (tmp_path / "x.d.fastq").read_bytes() == b"ACGT\nTTTT\nids\n@a\n@b\nquality\nHHHH\nIIII\n"
        assert not (tmp_path / "x.dna.d").exists() and not (tmp_path / "output").exists()
        log.unlink(); (tmp_path / "x.d.fastq").unlink()
        for f in os.listdir(tmp_path / "src"):
            (tmp_path / "src" / f).unlink()
        (tmp_path / "src").rmdir()


def test_d_without_q_still_writes_dna_d(tmp_path):
    env, log = _setup(tmp_path)
    r = _run(["-d", str(tmp_path / "x.harc")], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "x.dna.d").read_bytes() == b"ACGT\nTTTT\n" and not (tmp_path / "x.d.fastq").exists()
    assert [l.split()[0] for l in log.read_text().splitlines()] == ["decoder"]


def test_usage_names_the_fastq_output_and_its_caveat():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and ".d.fastq" in r.stdout and "byte for byte" in r.stdout and "without reads containing N" in r.stdout
