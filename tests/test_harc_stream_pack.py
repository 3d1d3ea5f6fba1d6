"""./harc -c -S and the .hs branch of ./harc -d without a GPU: the stage binary is replaced by a stand-in whose streams_pack / streams_unpack copy their files
and log their arguments, so that what is tested is the script's own work -- one call with exactly the expected pairs after the stage program has exited, the
members of the archive, the bytes the decoder is handed, a failing call, and the three refusals."""
import hashlib
import os
import stat
import subprocess
import tarfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = r"""#!/bin/bash
# stand-in for harc_amd_stage: fixed stream files in, checksums out; the stream packer copies and keeps a log
set -e
cmd=$1; base=$2; out=$base/output
case $cmd in
compressfq)
    E=$5
    for ((e = 0; e < E; e++)); do
        for s in read_seq read_pos read_noise read_noisepos read_rev; do head -c $((20000 + 977 * e)) /dev/zero | tr '\0' 'A' > $out/$s.txt.$e; done
        printf 'AC' > $out/read_seq.txt.$e.tail; printf '1' > $out/read_rev.txt.$e.tail
    done
    printf 'ACGTACGT\n' > $out/input_N.dna; printf 'clean\n' > $out/input_clean.dna
    head -c 5000 /dev/zero | tr '\0' 'G' > $out/read_singleton.txt; printf 'T' > $out/read_singleton.txt.tail
    printf '100\n' > $out/read_meta.txt
    for s in read_order.bin read_order_N.bin read_order_N_pe.bin numreads.bin read_order.bin.singleton temp.dna.singleton; do head -c 4000 /dev/urandom > $out/$s; done
    echo "Reordering done, 0 were unmatched"
    ls $out > $STUB_LOG.at_exit;;                                 # what is there when the stage program exits: no tar yet
pack_order) printf 'tail' > $out/read_order.bin.tail;;
streams_pack|streams_unpack)
    echo "$@" >> $STUB_LOG
    [ -n "$STUB_FAIL" ] && [ $cmd = streams_pack ] && exit 7
    shift 2
    while (( $# )); do
        if [ $cmd = streams_pack ]; then { printf 'HS'; cat "$1"; } > "$2"; else tail -c +3 "$1" > "$2"; fi
        shift 2
    done;;
decoder|decoder_preserve)
    (cd $out && find . -type f ! -name 'output.dna' | sort | xargs sha256sum) > $out/output.dna;;
*) echo "stub: unknown command $cmd"; exit 1;;
esac
"""

STREAMS = ["read_seq.tar", "read_pos.tar", "read_noise.tar", "read_noisepos.tar", "read_rev.tar", "input_N.dna", "read_singleton.txt"]
ORDER = ["read_order.bin", "read_order_N.bin", "read_order_N_pe.bin"]


def _setup(tmp_path):
    stub = tmp_path / "stage_stub.sh"
    stub.write_text(STUB)
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    fq = tmp_path / "s.fastq"
    fq.write_bytes(b"@a\n" + b"ACGT" * 25 + b"\n+\n" + b"H" * 100 + b"\n")
    env = dict(os.environ, HARC_AMD_STAGE_BIN=str(stub), STUB_LOG=str(tmp_path / "stub.log"))
    env.pop("HARC_AMD_STAGE3", None)
    return fq, env


def _run(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.mark.parametrize("flags", [[], ["-p"], ["-p", "-t", "3"], ["-t", "3"]])
def test_stream_pack_roundtrip(flags, tmp_path):
    fq, env = _setup(tmp_path)
    r = _run(["-c", str(fq), "-S"] + flags, env)
    assert r.returncode == 0, r.stdout[-2000:]
    arc, out = tmp_path / "s.harc", str(tmp_path / "output")
    assert arc.exists() and not (tmp_path / "output").exists()
    # one call, after the stage program has exited, with exactly the expected pairs in their order
    assert not [n for n in (tmp_path / "stub.log.at_exit").read_text().split() if n.endswith(".tar") or n.endswith(".hs")]
    log = (tmp_path / "stub.log").read_text().splitlines()
    want = STREAMS + (ORDER if "-p" in flags else [])
    assert log == ["streams_pack 0 " + " ".join("%s/%s %s/%s.hs" % (out, s, out, s) for s in want)], log
    with tarfile.open(arc) as tf:
        names = sorted(os.path.basename(n) for n in tf.getnames() if os.path.basename(n) not in ("", "."))
    for s in want:
        assert s + ".hs" in names and s not in names, names                            # the .hs set, and no raw stream is left
    assert "read_meta.txt" in names and "read_singleton.txt.tail" in names             # left raw, as in the xz branch
    assert "input_clean.dna" not in names and "temp.dna.singleton" not in names and "numreads.bin" not in names
    assert not [n for n in names if n.endswith(".xz")]
    if "-p" in flags:
        assert "read_order.bin.tail" in names
    else:
        assert not [n for n in names if n.startswith("read_order")]
    # -d finds the .hs files by itself: every file the decoder sees is what the encoder wrote (the stand-in decoder lists their checksums)
    r = _run(["-d", str(arc)] + (["-p"] if "-p" in flags else []), env)
    assert r.returncode == 0, r.stdout[-2000:]
    log = (tmp_path / "stub.log").read_text().splitlines()
    args = log[1].split()
    assert len(log) == 2 and args[:2] == ["streams_unpack", "0"], log
    assert sorted(zip(args[2::2], args[3::2])) == sorted(("%s/%s.hs" % (out, s), "%s/%s" % (out, s)) for s in want), log      # (in the order of the shell's glob)
    sums = dict(reversed(l.split(None, 1)) for l in (tmp_path / "s.dna.d").read_text().splitlines())
    E = int(flags[flags.index("-t") + 1]) if "-t" in flags else 8
    for e in range(E):
        for st in ["read_seq", "read_pos", "read_noise", "read_noisepos", "read_rev"]:
            assert sums[f"./{st}.txt.{e}"] == hashlib.sha256(b"A" * (20000 + 977 * e)).hexdigest()
        assert sums[f"./read_seq.txt.{e}.tail"] == hashlib.sha256(b"AC").hexdigest() and f"./read_rev.txt.{e}.tail" in sums
    assert sums["./input_N.dna"] == hashlib.sha256(b"ACGTACGT\n").hexdigest()
    assert sums["./read_singleton.txt"] == hashlib.sha256(b"G" * 5000).hexdigest()
    assert sums["./read_meta.txt"] == hashlib.sha256(b"100\n").hexdigest()
    assert not [k for k in sums if k.endswith(".hs")]


def test_a_failing_streams_pack_fails_the_run(tmp_path):
    fq, env = _setup(tmp_path)
    env["STUB_FAIL"] = "1"
    r = _run(["-c", str(fq), "-S"], env)
    assert r.returncode != 0 and "packing the streams on the GPU failed" in r.stdout, r.stdout[-1000:]
    assert not (tmp_path / "s.harc").exists() and not (tmp_path / "output").exists()


def test_the_three_refusals_come_before_anything_is_computed(tmp_path):
    fq, env = _setup(tmp_path)
    marker = tmp_path / "stub.log.at_exit"
    # -S with -d
    (tmp_path / "s.harc").write_bytes(b"")
    r = _run(["-d", str(tmp_path / "s.harc"), "-S"], env)
    assert r.returncode != 0 and "-S goes with -c only" in r.stdout, r.stdout[-1000:]
    (tmp_path / "s.harc").unlink()
    # -S beside a host packer
    for packer in ("xz", "none", "bsc", "zip"):
        r = _run(["-c", str(fq), "-S"], dict(env, HARC_AMD_STAGE3=packer))
        assert r.returncode != 0 and "HARC_AMD_STAGE3=%s does not go with it" % packer in r.stdout, r.stdout[-1000:]
    # -S without the stage program
    r = _run(["-c", str(fq), "-S"], dict(env, HARC_AMD_STAGE_BIN=str(tmp_path / "not_built")))
    assert r.returncode != 0 and "-S needs harc_amd_stage, which is not built" in r.stdout, r.stdout[-1000:]
    assert not marker.exists() and not (tmp_path / "output").exists() and not (tmp_path / "s.harc").exists() and not (tmp_path / "stub.log").exists()
    # auto is what -S goes with
    r = _run(["-c", str(fq), "-S"], dict(env, HARC_AMD_STAGE3="auto"))
    assert r.returncode == 0 and (tmp_path / "s.harc").exists(), r.stdout[-1000:]
    r = _run(["-h"], env)
    assert "[-S]" in r.stdout and "-S Only with -c" in r.stdout
