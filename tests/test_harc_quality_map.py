"""./harc -c -q -b SPEC without a GPU: the stage binary is replaced by a stand-in that logs how it was called.  What is tested is the script's own work: that -b
anywhere else is refused before anything is computed, and a spec that `quality_spec` rejects before output/ is made; that with -Q the spec rides on the one
`quality_pack` call and nothing else maps; that without -Q `quality_map` writes X.quality.tmp, which then replaces X.quality; that a failing call leaves
X.quality as it was, no .tmp and no output/; that without -b the calls are exactly what they were; and that the usage text names it."""
import os
import stat
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTQ = b"@a\nACGT\n+\nHHHH\n@b\nTTTT\n+\nIIII\n"

STUB = r"""#!/bin/bash
# stand-in for harc_amd_stage: logs its arguments, writes what the real stages would leave
set -e
echo "$@" >> "$STUB_LOG"
case $1 in
quality_spec) case $2 in ill8|pblock:2|cap:30) exit 0;; *) echo "stub: no spec $2" >&2; exit 2;; esac;;
compressfq)
	o=$2/output
	for s in read_seq read_pos read_noise read_noisepos read_rev; do echo x > $o/$s.txt.0; done
	echo x > $o/input_N.dna; echo x > $o/read_singleton.txt; echo 4 > $o/read_meta.txt; echo x > $o/read_order.bin; echo x > $o/numreads.bin
	printf 'HHHH\nIIII\n' > $o/output.quality; printf '@a\n@b\n' > $o/output.id;;
pack_order) ;;
quality_pack) [ -z "$STUB_FAIL_PACK" ] || exit 1; { echo "packed $5"; cat "$2"; } > "$4";;
quality_map) if [ -n "$STUB_FAIL_MAP" ]; then echo half > "$4"; exit 1; fi; { echo "mapped $5"; cat "$2"; } > "$4";;
id_pack) { echo ids; cat "$2"; } > "$4";;
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


def test_b_without_q_or_with_d_or_with_a_bad_spec_is_refused_before_anything_is_computed(tmp_path):
    env, log = _setup(tmp_path)
    fq = str(tmp_path / "in.fastq")
    for flags in (["-b", "ill8"], ["-p", "-b", "ill8"], ["-b", "nonsense"]):                 # without -q: refused before the spec is even looked at
        r = _run(["-c", fq] + flags, env)
        assert r.returncode != 0 and "-b" in r.stdout and "-q" in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "in.harc").exists()
    (tmp_path / "x.harc").write_bytes(b"")
    (tmp_path / "x.id").write_bytes(b"@a\n@b\n")
    (tmp_path / "x.quality").write_bytes(b"HHHH\nIIII\n")
    for flags in (["-b", "ill8"], ["-q", "-b", "ill8"], ["-p", "-q", "-b", "nonsense"]):     # with -d
        r = _run(["-d", str(tmp_path / "x.harc")] + flags, env)
        assert r.returncode != 0 and "-b" in r.stdout and "-c -q" in r.stdout, r.stdout[-2000:]
        assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "x.d.fastq").exists()
    # in the words of the -Q refusals
    rb, rq = _run(["-c", fq, "-b", "ill8"], env), _run(["-c", fq, "-Q"], env)
    assert rb.stdout.startswith("-b needs -q: only the quality values that -c -q writes can be ") and rq.stdout.startswith("-Q needs -q: only the quality values that -c -q writes can be ")
    # a spec that quality_spec rejects: that one call, its reason, and nothing else
    for flags in (["-q", "-b", "bin:1"], ["-q", "-Q", "-b", "bin:1"], ["-p", "-q", "-I", "-b", "bin:1"]):
        r = _run(["-c", fq] + flags, env)
        assert r.returncode == 1 and "stub: no spec bin:1" in r.stdout and "bin:1" in r.stdout.splitlines()[-1], r.stdout[-2000:]
        assert _calls(log) == [["quality_spec", "bin:1"]]
        assert not (tmp_path / "output").exists() and not (tmp_path / "in.harc").exists() and not (tmp_path / "in.quality").exists()
        os.remove(log)


def test_with_Q_the_spec_goes_to_the_one_quality_pack_call(tmp_path):
    for k, flags in enumerate((["-q", "-Q", "-b", "ill8"], ["-p", "-b", "ill8", "-q", "-Q"], ["-q", "-Q", "-I", "-b", "ill8"])):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d)
        r = _run(["-c", str(d / "in.fastq")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = _calls(log)
        assert [c[0] for c in calls][:3] == ["quality_spec", "compressfq", "quality_pack"] and calls[0] == ["quality_spec", "ill8"]
        assert [c for c in calls if c[0] == "quality_pack"] == [["quality_pack", str(d / "in.quality"), "0", str(d / "in.quality.hq"), "ill8"]], calls
        assert not [c for c in calls if c[0] == "quality_map"]
        assert (d / "in.quality.hq").read_bytes() == b"packed ill8\nHHHH\nIIII\n" and not (d / "in.quality").exists() and not (d / "in.quality.tmp").exists()
        assert (d / "in.harc").exists() and not (d / "output").exists()
        if "-I" in flags:                                          # -I is independent
            assert ["id_pack", str(d / "in.id"), "0", str(d / "in.id.hi")] in calls and (d / "in.id.hi").exists()
        else:
            assert (d / "in.id").read_bytes() == b"@a\n@b\n"


def test_without_Q_quality_map_writes_a_tmp_file_that_replaces_the_quality_file(tmp_path):
    for k, flags in enumerate((["-q", "-b", "pblock:2"], ["-p", "-q", "-b", "pblock:2"], ["-b", "pblock:2", "-I", "-q"])):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d)
        r = _run(["-c", str(d / "in.fastq")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = _calls(log)
        assert [c[0] for c in calls][:3] == ["quality_spec", "compressfq", "quality_map"]
        assert calls[2] == ["quality_map", str(d / "in.quality"), "0", str(d / "in.quality.tmp"), "pblock:2"], calls
        assert not [c for c in calls if c[0] == "quality_pack"]
        assert (d / "in.quality").read_bytes() == b"mapped pblock:2\nHHHH\nIIII\n" and not (d / "in.quality.tmp").exists() and not (d / "in.quality.hq").exists()
        assert (d / "in.harc").exists() and not (d / "output").exists()


def test_a_failing_call_leaves_the_quality_file_and_nothing_else(tmp_path):
    for k, (flags, fail) in enumerate(((["-q", "-b", "ill8"], "STUB_FAIL_MAP"), (["-q", "-Q", "-b", "ill8"], "STUB_FAIL_PACK"))):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d)
        r = _run(["-c", str(d / "in.fastq")] + flags, dict(env, **{fail: "1"}))
        assert r.returncode == 1, r.stdout[-2000:]
        assert (d / "in.quality").read_bytes() == b"HHHH\nIIII\n"
        assert not (d / "in.quality.tmp").exists() and not (d / "in.quality.hq").exists() and not (d / "output").exists() and not (d / "in.harc").exists()


def test_without_b_the_calls_are_what_they_were(tmp_path):
    for k, (flags, want) in enumerate(((["-q"], ["compressfq"]), (["-q", "-Q"], ["compressfq", "quality_pack"]), (["-p", "-q", "-Q", "-I"], ["compressfq", "quality_pack", "id_pack", "pack_order"]))):
        d = tmp_path / str(k)
        d.mkdir()
        env, log = _setup(d)
        r = _run(["-c", str(d / "in.fastq")] + flags, env)
        assert r.returncode == 0, r.stdout[-2000:]
        calls = _calls(log)
        assert [c[0] for c in calls] == want, calls
        for c in calls:
            if c[0] == "quality_pack":
                assert c == ["quality_pack", str(d / "in.quality"), "0", str(d / "in.quality.hq")]                 # four words: no spec, not even an empty one
        if "-Q" in flags:
            assert (d / "in.quality.hq").read_bytes() == b"packed \nHHHH\nIIII\n"
        else:
            assert (d / "in.quality").read_bytes() == b"HHHH\nIIII\n"


def test_usage_names_b_and_the_four_specs():
    r = subprocess.run([os.path.join(ROOT, "harc"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0
    for word in ("-b spec", "[-b spec]", "ill8", "bin:T:H:L", "cap:M", "pblock:R", "irreversibl"):
        assert word in r.stdout, word
