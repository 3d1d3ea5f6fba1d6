"""./harc -c -P and -R without a GPU: the stage binary is replaced by a stand-in that logs how it was called.  What is tested is the script's own work: that -P
anywhere but at -c, a percentage that is none, and -n without -R are refused before anything is computed; that recovery_make is the last call of a run, over the
files that exist at that moment; that a run without -P calls nothing new; that a failing recovery_make leaves the archive and no X.hr; the calls and statuses of -R."""
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
compressfq)
	o=$2/output
	for s in read_seq read_pos read_noise read_noisepos read_rev; do echo x > $o/$s.txt.0; done
	echo x > $o/input_N.dna; echo x > $o/read_singleton.txt; echo 4 > $o/read_meta.txt; echo x > $o/read_order.bin; echo x > $o/numreads.bin
	echo x > $o/read_order_N.bin; echo x > $o/read_order_N_pe.bin
	printf 'HHHH\nIIII\n' > $o/output.quality; printf '@a\n@b\n' > $o/output.id;;
pack_order) ;;
quality_pack) { echo packed; cat "$2"; } > "$4";;
id_pack) { echo ids; cat "$2"; } > "$4";;
recovery_make)
	[ -d "$(dirname "$4")/output" ] && { echo "stub: output/ is still there"; exit 1; }
	shift 3; out=$1; shift
	for f in "$@"; do [ -f "$f" ] || { echo "stub: $f is missing"; exit 1; }; done
	echo half > "$out"
	[ -z "$STUB_BAD_RECOVERY" ] || { echo "stub: recovery_make fails" >&2; exit 1; }
	echo record > "$out"
	echo "[recovery] $# files, 1 bytes protected, 2 bytes of $out, 3 blocks, 4 groups";;
recovery_check|recovery_repair) echo "[recovery] in.harc ${STUB_R_WORD:-ok}"; exit ${STUB_R_STATUS:-0};;
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


def test_the_refusals_come_before_any_stage_call(tmp_path):
    env, log = _setup(tmp_path)
    fq, arc = str(tmp_path / "in.fastq"), str(tmp_path / "x.harc")
    (tmp_path / "x.harc").write_bytes(b"")
    (tmp_path / "x.hr").write_bytes(b"")
    for mode in ("-d", "-v", "-R"):
        for flags in (["-P", "5"], ["-p", "-P", "100"]):
            r = _run([mode, arc] + flags, env)
            assert r.returncode == 1 and r.stdout.startswith("-P goes with -c only (it "), r.stdout[-2000:]
    for pct in ("0", "101", "5.5", "-3", "ten", "", "1000", "5x"):
        r = _run(["-c", fq, "-P", pct], env)
        assert r.returncode == 1 and r.stdout.startswith("-P %s: not a percentage" % pct), (pct, r.stdout[-2000:])
    for args in (["-c", fq, "-n"], ["-d", arc, "-n"], ["-v", arc, "-n"]):
        r = _run(args, env)
        assert r.returncode == 1 and r.stdout.startswith("-n goes with -R only (it "), r.stdout[-2000:]
    # two modes give the usage text, as -c with -d does, and the usage text names both
    both = _run(["-c", fq, "-d", arc], env)
    for args in (["-R", arc, "-c", fq], ["-d", arc, "-R", arc], ["-R", arc, "-v", arc]):
        r = _run(args, env)
        assert r.stdout == both.stdout and r.returncode == both.returncode and "-R HARC_file [-n]" in r.stdout and "[-P percent]" in r.stdout
    # no record next to the archive
    (tmp_path / "x.hr").unlink()
    for flags in ([], ["-n"]):
        r = _run(["-R", arc] + flags, env)
        assert r.returncode == 1 and "was not compressed with -P" in r.stdout
    assert not log.exists() and not (tmp_path / "output").exists() and not (tmp_path / "in.harc").exists()


def test_recovery_make_is_the_last_call_over_the_files_that_exist(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(["-c", str(d / "in.fastq"), "-p", "-q", "-Q", "-I", "-P", "5"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    calls = _calls(log)
    x = str(d / "in")
    assert calls[-1] == ["recovery_make", "5", "0", x + ".hr", x + ".harc", x + ".quality.hq", x + ".id.hi"]      # the packed files, not the texts
    assert [c[0] for c in calls].count("recovery_make") == 1
    assert (d / "in.hr").read_text() == "record\n" and (d / "in.harc").exists() and not (d / "output").exists()
    assert "[recovery] 3 files" in r.stdout
    # the texts, when they are what the run left; -P 007 is the number 7
    for f in ("in.hr", "in.harc", "in.quality.hq", "in.id.hi"):
        (d / f).unlink()
    log.unlink()
    r = _run(["-c", str(d / "in.fastq"), "-q", "-P", "007"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert _calls(log)[-1] == ["recovery_make", "7", "0", x + ".hr", x + ".harc", x + ".quality", x + ".id"]
    # without -q: the archive alone
    for f in ("in.hr", "in.harc", "in.quality", "in.id"):
        (d / f).unlink()
    log.unlink()
    assert _run(["-c", str(d / "in.fastq"), "-P", "100"], env).returncode == 0
    assert _calls(log)[-1] == ["recovery_make", "100", "0", x + ".hr", x + ".harc"]


def test_without_P_nothing_changes(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(["-c", str(d / "in.fastq"), "-p", "-q", "-Q", "-I"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert [c[0] for c in _calls(log)] == ["compressfq", "quality_pack", "id_pack", "pack_order"]
    assert not (d / "in.hr").exists() and "[recovery]" not in r.stdout


def test_a_failing_recovery_make_leaves_the_archive_and_no_record(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    r = _run(["-c", str(d / "in.fastq"), "-p", "-q", "-Q", "-I", "-P", "5"], dict(env, STUB_BAD_RECOVERY="1"))
    assert r.returncode == 1, r.stdout[-2000:]
    assert "could not be written" in r.stdout and "stay" in r.stdout
    assert not (d / "in.hr").exists() and not (d / "output").exists()
    for f in ("in.harc", "in.quality.hq", "in.id.hi"):
        assert (d / f).exists(), f


def test_the_calls_and_statuses_of_R(tmp_path):
    env, log = _setup(tmp_path)
    d = tmp_path
    (d / "in.harc").write_bytes(b"x")
    (d / "in.hr").write_bytes(b"x")
    r = _run(["-R", str(d / "in.harc")], env)
    assert r.returncode == 0 and r.stdout == "[recovery] in.harc ok\n"
    r = _run(["-R", str(d / "in.harc"), "-n"], env)
    assert r.returncode == 0 and r.stdout == "[recovery] in.harc ok\n"
    r = _run(["-n", "-R", str(d / "in.harc")], dict(env, STUB_R_STATUS="1", STUB_R_WORD="damaged"))
    assert r.returncode == 1 and r.stdout == "[recovery] in.harc damaged\n"
    r = _run(["-R", str(d / "in.harc")], dict(env, STUB_R_STATUS="1", STUB_R_WORD="NOT recoverable"))
    assert r.returncode == 1 and "NOT recoverable" in r.stdout
    hr = str(d / "in.hr")
    assert _calls(log) == [["recovery_repair", hr, "0"], ["recovery_check", hr, "0"], ["recovery_check", hr, "0"], ["recovery_repair", hr, "0"]]
    assert not (d / "output").exists()
    # -d and -v do not consult the record: they are what they were (here: they fail on the empty archive, without a recovery call)
    log.unlink()
    _run(["-v", str(d / "in.harc")], env)
    assert not log.exists() or all(not c[0].startswith("recovery") for c in _calls(log))
