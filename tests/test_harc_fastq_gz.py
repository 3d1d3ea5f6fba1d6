"""./harc -d -q -z without a GPU: the stage binary is replaced by a stand-in that logs how it was called.  What is tested is the script's own work: that -z
sends the decoder's output through `fastq_out` with the five paths, the last being X.d.fastq.gz, followed by `bgzf`; that -z anywhere else is refused before
anything is unpacked; and that the usage text names it."""
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
    env = dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), STUB_LOG=str(log))
    return env, log


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_d_q_z_runs_the_decoder_and_then_fastq_out_with_bgzf(tmp_path):
    for k, (flags, dec) in enumerate(((["-q", "-z"], "decoder"), (["-p", "-q", "-z"], "decoder_preserve"), (["-z", "-q"], "decoder"))):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d, order=dec == "decoder_preserve")
        (d / "x.id").write_bytes(b"@a\n@b\n")
        (d / "x.quality").write_bytes(b"HHHH\nIIII\n")
        r = _run(["-d", str(d / "x.harc")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = [l.split() for l in log.read_text().splitlines()]
        assert [c[0] for c in calls] == [dec, "fastq_out"], calls
        out = str(d / "output")
        assert calls[1][1:] == [out + "/output.dna", "0", str(d / "x.id"), str(d / "x.quality"), str(d / "x.d.fastq.gz"), "bgzf"], calls[1]
        assert (d / "x.d.fastq.gz").read_bytes() == b"ACGT\nTTTT\nids\n@a\n@b\nquality\nHHHH\nIIII\nmode=bgzf\n"
        assert not (d / "x.d.fastq").exists() and not (d / "x.dna.d").exists() and not (d / "output").exists()


def test_z_without_q_or_with_c_is_refused_before_anything_is_unpacked(tmp_path):
    env, log = _setup(tmp_path)
    (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
    (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
    r = _run(["-d", str(tmp_path / "x.harc"), "-z"], env)
    assert r.returncode != 0 and "-z" in r.stdout and "-q" in r.stdout, r.stdout[-2000:]
    assert not log.exists() and not (tmp_path / "output").exists()
    assert not (tmp_path / "x.d.fastq.gz").exists() and not (tmp_path / "x.dna.d").exists()
    (tmp_path / "in.fastq").write_bytes(b"@a\nACGT\n+\nHHHH\n")
    for flags in (["-z"], ["-q", "-z"], ["-p", "-q", "-z"]):
        r = _run(["-c", str(tmp_path / "in.fastq")] + flags, env)
        assert r.returncode != 0 and "-z" in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "in.harc").exists()


def test_usage_names_the_gzipped_output():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("-z", ".d.fastq.gz", "BGZF", "bgzip -d", "gzip -d", "samtools", "./harc -c"):
        assert word in r.stdout, word
