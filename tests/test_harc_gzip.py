"""./harc -c on gzip input without a GPU: the stage binary is replaced by a stand-in that records the file each command receives.  BGZF goes
to the stage program as it is (the GPU inflates it), any other gzip -- and any gzip with -g -- is expanded on the host first into
output/.input.fastq, which never reaches the archive; the read length is read through gzip; the archive is named without .gz / .fastq."""
import gzip
import os
import stat
import subprocess
import tarfile

from tests import bgzf_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = r"""#!/bin/bash
# stand-in for harc_amd_stage: records the command, the read length and a copy of the input it was given
set -e
cmd=$1; base=$2; out=$base/output
streams()
{
    for s in read_seq read_pos read_noise read_noisepos read_rev; do printf 'AAAA' > $out/$s.txt.0; done
    printf 'AC' > $out/read_seq.txt.0.tail; printf '1' > $out/read_rev.txt.0.tail
    printf 'ACGT\n' > $out/input_N.dna; printf 'G' > $out/read_singleton.txt; printf 'T' > $out/read_singleton.txt.tail
    printf '100\n' > $out/read_meta.txt
    for s in read_order.bin read_order_N.bin read_order_N_pe.bin numreads.bin; do printf 'xxxx' > $out/$s; done
}
case $cmd in
compressfq|compressfq_shard)
    echo "$cmd $3 $4" >> "$STUB_LOG"
    cp "$4" "$STUB_LOG.$cmd.input${11:+.${11}}"                  # ranks of -g run side by side: one copy each (rank = 11th argument)
    [[ $cmd == compressfq ]] && streams
    exit 0;;
merge_shards) streams;;
pack_order) printf 'tail' > $out/read_order.bin.tail;;
*) echo "stub: unknown command $cmd"; exit 1;;
esac
"""


def _setup(tmp_path):
    stub = tmp_path / "stage_stub.sh"
    stub.write_text(STUB)
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    text = bu.fastq_text(300, 100, seed=1)
    env = dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), HARC_AMD_STAGE3="none", STUB_LOG=str(tmp_path / "stub.log"))
    return text, env


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _names(arc):
    with tarfile.open(arc) as tf:
        return sorted(os.path.basename(n) for n in tf.getnames() if os.path.basename(n) not in ("", "."))


def test_bgzf_goes_to_the_stage_program_as_it_is(tmp_path):
    text, env = _setup(tmp_path)
    gz = tmp_path / "x.fastq.gz"
    gz.write_bytes(bu.bgzf(text, 4099))
    r = _run(["-c", str(gz)], env)
    assert r.returncode == 0, r.stdout[-2000:]
    cmd, readlen, got = (tmp_path / "stub.log").read_text().split()
    assert (cmd, readlen, got) == ("compressfq", "100", str(gz))
    assert (tmp_path / "stub.log.compressfq.input").read_bytes() == gz.read_bytes()
    assert (tmp_path / "x.harc").exists() and not (tmp_path / "output").exists()
    assert "read_meta.txt" in _names(tmp_path / "x.harc")


def test_plain_gzip_is_expanded_on_the_host_and_left_out_of_the_archive(tmp_path):
    text, env = _setup(tmp_path)
    gz = tmp_path / "y.fq.gz"                                     # the name says nothing: the magic bytes decide
    gz.write_bytes(gzip.compress(text))
    r = _run(["-c", str(gz)], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "bgzip" in r.stdout
    cmd, readlen, got = (tmp_path / "stub.log").read_text().split()
    assert cmd == "compressfq" and readlen == "100" and got.endswith("output/.input.fastq")
    assert (tmp_path / "stub.log.compressfq.input").read_bytes() == text
    names = _names(tmp_path / "y.fq.harc")
    assert ".input.fastq" not in names and "read_meta.txt" in names
    assert not (tmp_path / "output").exists()


def test_multi_gpu_expands_bgzf_first(tmp_path):
    text, env = _setup(tmp_path)
    gz = tmp_path / "z.fastq.gz"
    gz.write_bytes(bu.bgzf(text, 4099))
    r = _run(["-c", str(gz), "-g", "2", "-p"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = (tmp_path / "stub.log").read_text().splitlines()
    assert len(lines) == 2 and all(l.startswith("compressfq_shard 100 ") and l.endswith("output/.input.fastq") for l in lines), lines
    assert (tmp_path / "stub.log.compressfq_shard.input.0").read_bytes() == text
    assert (tmp_path / "stub.log.compressfq_shard.input.1").read_bytes() == text
    assert ".input.fastq" not in _names(tmp_path / "z.harc")


def test_plain_fastq_names_do_not_change(tmp_path):
    text, env = _setup(tmp_path)
    fq = tmp_path / "w.fastq"
    fq.write_bytes(text)
    r = _run(["-c", str(fq)], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "stub.log").read_text().split() == ["compressfq", "100", str(fq)]
    assert (tmp_path / "w.harc").exists()
