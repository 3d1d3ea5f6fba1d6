"""The recovery record on the GPU (./harc -c -P, -R; README: "-P and what it promises").  The block digest and combine kernels against the host twin and the plain
Python reference at every case of tests/recovery_cases.py; the file calls against the reference's record and the reference's repairs, whatever the slices of the
ring; and ./harc -c -P, -R -n, -R, -d end to end on a small input."""
import os
import random
import subprocess

import pytest

from tests import gen
from tests import id_cases
from tests import quality_cases as qc
from tests import recovery_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


@pytest.fixture(scope="module")
def cases():
    return rc.cases()


@pytest.fixture(scope="module")
def records(cases):
    """the reference's record of every case, made once"""
    return {c["name"]: rc.make_record(c["files"], c["PCT"], c["B"], c["S"], c["K"]) for c in cases}


def _on_device(b, room):
    """b at the start of an allocation of `room` bytes, 0xA5 behind it -> (tensor, device address)"""
    import torch
    t = torch.full((room + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    if b:
        t[:len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()                                          # the library works on a stream of its own
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


def _geometry(monkeypatch, c):
    monkeypatch.setenv("HARC_AMD_RECOVERY_BLOCK", str(c["B"]))
    monkeypatch.setenv("HARC_AMD_RECOVERY_SPAN", str(c["S"]))
    monkeypatch.setenv("HARC_AMD_RECOVERY_GROUP", str(c["K"]))


# ------------------------------------------------------------------------------------------------ the kernels
def test_the_device_digests_are_the_host_twins_at_every_case(ctx, cases):
    import harc_amd
    for c in cases:
        B = c["B"]
        for name, data in c["files"]:
            nb = -(-len(data) // B)
            if not nb:
                assert ctx.block_digests_device(0, 0, B) == []
                continue
            t, p = _on_device(data, nb * B)                         # what lies behind a short last block is not zero: it must not be counted
            want = [rc.digest(b) for b in rc.blocks_of(data, B)]
            assert harc_amd.block_digests_host(data, B) == want
            assert ctx.block_digests_device(p, nb, B, len(data) - (nb - 1) * B) == want, (c["name"], name)
    # more blocks than one, each more than one trip of a workgroup, the last one byte long
    data = rc._bytes("digests", 5 * 8208 + 1)
    t, p = _on_device(data, 6 * 8208)
    assert ctx.block_digests_device(p, 6, 8208, 1) == [rc.digest(b) for b in rc.blocks_of(data, 8208)]
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.block_digests_device(p + 8, 1, 16)
    assert e.value.code == EINVAL
    with pytest.raises(harc_amd.HarcAmdError):
        ctx.block_digests_device(p, 1, 24)


def _combine_on_device(ctx, sources, coef):
    import torch
    B, ns, e = len(sources[0]), len(sources), len(coef)
    t, p = _on_device(b"".join(sources), (ns + e) * B)
    ctx.gf_combine_device(B, [p + s * B for s in range(ns)], [p + (ns + q) * B for q in range(e)], coef)
    torch.cuda.synchronize()
    got = bytes(t.cpu().numpy().tobytes())
    assert got[:ns * B] == b"".join(sources) and got[(ns + e) * B:] == b"\xa5" * 64       # no byte outside the outputs is written
    return [got[(ns + q) * B:(ns + q + 1) * B] for q in range(e)]


def test_the_device_combine_is_the_host_twins_at_every_case(ctx, cases):
    import harc_amd
    for c in cases:
        B = c["B"]
        for name, data in c["files"]:
            blocks = rc.blocks_of(data, B)
            if not blocks:
                continue
            G, groups = rc.groups_of_span(min(len(blocks), c["S"]), c["K"], c["PCT"])
            k, m = groups[0]
            members = [rc.pad(blocks[j * G], B) for j in range(k)]
            coef = [[rc.cauchy(i, j) for j in range(k)] for i in range(m)]
            want = rc.combine(members, coef)
            assert harc_amd.gf_combine_host(members, coef) == want
            assert _combine_on_device(ctx, members, coef) == want, (c["name"], name)
    # a block of more chunks than a workgroup has lanes, nine outputs (two passes, the second of one), every coefficient bit
    rnd = random.Random(3)
    B = 16 * 300
    sources = [rc._bytes("combine%d" % s, B) for s in range(3)]
    coef = [[rnd.getrandbits(8) for _ in range(3)] for _ in range(7)] + [[0, 0, 0], [255, 1, 128]]
    assert _combine_on_device(ctx, sources, coef) == rc.combine(sources, coef) == harc_amd.gf_combine_host(sources, coef)
    t, p = _on_device(b"", 64)
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.gf_combine_device(16, [p + 4], [p + 32], [[1]])
    assert e.value.code == EINVAL


# ------------------------------------------------------------------------------------------------ the file calls
def _lay_out(d, case, files=None, rec=None):
    d.mkdir(exist_ok=True)
    files = dict(case["files"]) if files is None else files
    paths = []
    for name, _ in case["files"]:
        p = d / name
        if files.get(name) is None:
            if p.exists():
                p.unlink()
        else:
            p.write_bytes(files[name])
        paths.append(str(p))
    if rec is not None:
        (d / "x.hr").write_bytes(rec)
    return paths, str(d / "x.hr")


def test_recovery_make_files_writes_the_references_record_whatever_the_slices(tmp_path, monkeypatch, cases, records):
    import harc_amd
    for c in cases:
        _geometry(monkeypatch, c)
        paths, out = _lay_out(tmp_path / c["name"], c)
        st = harc_amd.recovery_make_files(paths, c["PCT"], out=out)
        assert open(out, "rb").read() == records[c["name"]], c["name"]
        assert st["record_bytes"] == len(records[c["name"]]) and st["bytes"] == sum(len(x) for _, x in c["files"])
        assert harc_amd.recovery_check_files(out) == (0, ["[recovery] %s ok" % n for n, _ in c["files"]])
    for c in (x for x in cases if x["name"] in ("b48", "spans3", "three")):      # slices of a few blocks, and of no whole block
        _geometry(monkeypatch, c)
        for sl, threads in (("48", "1"), ("40", "3")):
            monkeypatch.setenv("HARC_AMD_FEED_SLICE", sl)
            monkeypatch.setenv("HARC_AMD_FEED_THREADS", threads)
            paths, out = _lay_out(tmp_path / c["name"], c)
            os.remove(out)
            harc_amd.recovery_make_files(paths, c["PCT"], out=out)
            assert open(out, "rb").read() == records[c["name"]], (c["name"], sl, threads)
        monkeypatch.delenv("HARC_AMD_FEED_SLICE")
        monkeypatch.delenv("HARC_AMD_FEED_THREADS")
    with pytest.raises(harc_amd.HarcAmdError):                       # a failed call leaves no record
        harc_amd.recovery_make_files([str(tmp_path / "none.bin")], 5, out=str(tmp_path / "none.hr"))
    assert not (tmp_path / "none.hr").exists()


def _group_blocks(case, fi, g=0):
    data = case["files"][fi][1]
    nb = -(-len(data) // case["B"])
    G, groups = rc.groups_of_span(min(nb, case["S"]), case["K"], case["PCT"])
    k, m = groups[g]
    return [j * G + g for j in range(k)], k, m, G


def _damage(data, B, blocks):
    x = bytearray(data)
    for t in blocks:
        x[t * B + min(5, len(data) - t * B - 1)] ^= 0x21
    return bytes(x)


def _both(tmp, case, rec, files, write=True):
    """the reference and the GPU file call on the same damaged files -> (status, lines), after asserting that both agree on status, lines and bytes"""
    import harc_amd
    _, hr = _lay_out(tmp, case, files, rec)
    want = rc.repair(rec, "x.hr", files, write)
    got = (harc_amd.recovery_repair_files if write else harc_amd.recovery_check_files)(hr)
    assert got == want[:2], (got, want[:2])
    for name, _ in case["files"]:
        p = tmp / name
        assert (p.read_bytes() if p.exists() else None) == want[2].get(name), name
    assert open(hr, "rb").read() == rec
    return got


def test_recovery_repair_files_restores_what_can_be_and_refuses_the_rest_in_the_twins_words(tmp_path, cases, records):
    import harc_amd
    for c in cases:                                                # a flipped bit, then exactly m lost members of a group, in every case
        fi = max(range(len(c["files"])), key=lambda i: len(c["files"][i][1]))
        name, data = c["files"][fi]
        files = dict(c["files"])
        x = bytearray(data)
        x[len(x) // 2] ^= 1
        files[name] = bytes(x)
        assert _both(tmp_path / c["name"], c, records[c["name"]], files, write=False)[0] == 1
        assert _both(tmp_path / c["name"], c, records[c["name"]], files)[0] == 0
        blocks, k, m, G = _group_blocks(c, fi)
        files[name] = _damage(data, c["B"], blocks[-min(k, m):])
        st, lines = _both(tmp_path / c["name"], c, records[c["name"]], files)
        assert st == 0 and (tmp_path / c["name"] / name).read_bytes() == data, (c["name"], lines)
    # m + 1 lost in the first file: refused, its bytes unchanged -- and the same context goes on to repair the third file
    c = next(x for x in cases if x["name"] == "three")
    blocks, k, m, G = _group_blocks(c, 0)
    files = dict(c["files"])
    files["f0.bin"] = _damage(files["f0.bin"], c["B"], blocks[:m + 1])
    files["f2.bin"] = _damage(files["f2.bin"], c["B"], [1])
    st, lines = _both(tmp_path / "mixed", c, records["three"], files)
    assert st == 1 and lines == ["[recovery] f0.bin NOT recoverable: span 0 group 0 has lost %d of %d blocks and holds %d recovery blocks" % (m + 1, k, m),
                                 "[recovery] f1.bin ok", "[recovery] f2.bin repaired: 1 of 5 blocks"]
    assert (tmp_path / "mixed" / "f0.bin").read_bytes() == files["f0.bin"] and (tmp_path / "mixed" / "f2.bin").read_bytes() == c["files"][2][1]
    # a burst of G m blocks, and one more from a group boundary
    c = next(x for x in cases if x["name"] == "b48")
    name, data = c["files"][0]
    _, k, m, G = _group_blocks(c, 0)
    assert _both(tmp_path / "burst", c, records["b48"], {name: _damage(data, c["B"], range(1, 1 + G * m))})[0] == 0
    assert _both(tmp_path / "burst", c, records["b48"], {name: _damage(data, c["B"], range(0, G * m + 1))})[0] == 1
    # a damaged recovery block alone, with m - 1 lost members, and with m
    x = bytearray(records["b48"])
    x[rc.read_head(records["b48"])[0]["hb"] + 7] ^= 2
    rec = bytes(x)
    assert _both(tmp_path / "rb", c, rec, {name: data}) == (0, ["[recovery] x.hr: 1 of 4 recovery blocks damaged", "[recovery] %s ok" % name])
    blocks, k, m, G = _group_blocks(c, 0)
    assert _both(tmp_path / "rb", c, rec, {name: _damage(data, c["B"], blocks[:m - 1])})[0] == 0
    assert _both(tmp_path / "rb", c, rec, {name: _damage(data, c["B"], blocks[:m])})[0] == 1
    # a truncated file and a missing file at PCT = 100; a longer file
    c = next(x for x in cases if x["name"] == "m128")
    name, data = c["files"][0]
    for cut in (len(data) - 1, len(data) - 16 * 5 - 3, 0):
        assert _both(tmp_path / "cut", c, records["m128"], {name: data[:cut]})[0] == 0
    assert _both(tmp_path / "gone", c, records["m128"], {name: None}, write=False)[0] == 1
    assert _both(tmp_path / "gone", c, records["m128"], {name: None}) == (0, ["[recovery] %s repaired: 128 of 128 blocks" % name])
    _lay_out(tmp_path / "long", c, {name: data + b"!"}, records["m128"])
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.recovery_repair_files(str(tmp_path / "long" / "x.hr"))
    assert e.value.code == EINVAL and "holds 2049 bytes" in str(e.value) and (tmp_path / "long" / name).read_bytes() == data + b"!"
    # head copy one damaged; both
    one = bytearray(records["m128"])
    one[60] ^= 1
    assert _both(tmp_path / "head", c, bytes(one), {name: _damage(data, 16, [3])})[1][0] == "[recovery] x.hr: the first copy of the head is damaged, the second holds"
    one[len(one) - 20] ^= 1
    _lay_out(tmp_path / "head", c, {name: data}, bytes(one))
    with pytest.raises(harc_amd.HarcAmdError) as e:
        harc_amd.recovery_check_files(str(tmp_path / "head" / "x.hr"))
    assert e.value.code == EINVAL and "neither copy" in str(e.value)


# ------------------------------------------------------------------------------------------------ end to end
def _harc(args, env):
    return subprocess.run([os.path.join(ROOT, "harc")] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_harc_c_P_then_R_n_R_and_d_end_to_end(tmp_path):
    L, n = 100, 3000
    reads = gen.reads_text(141, n, L, 20000, err=0.01, n_frac=0.25).split()
    ids = id_cases.ids(n)
    quals = qc.markov(n, L, seed=17).split()
    fastq = b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))
    (tmp_path / "x.fastq").write_bytes(fastq)
    env = dict(os.environ, HARC_AMD_STAGE3="none", HARC_AMD_RECOVERY_BLOCK="1024")
    r = _harc(["-c", str(tmp_path / "x.fastq"), "-p", "-q", "-Q", "-I", "-t", "2", "-P", "10"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("[recovery]")]
    assert len(line) == 1 and line[0].startswith("[recovery] 3 files, "), r.stdout[-2000:]
    names = ("x.harc", "x.quality.hq", "x.id.hi")
    orig = {f: (tmp_path / f).read_bytes() for f in names}
    H, which = rc.read_head((tmp_path / "x.hr").read_bytes())
    assert which == 1 and [f["name"] for f in H["files"]] == list(names) and H["B"] == 1024 and H["PCT"] == 10
    assert [(f["n"], f["D"]) for f in H["files"]] == [(len(orig[f]), rc.digest(orig[f])) for f in names]
    assert _harc(["-R", str(tmp_path / "x.harc"), "-n"], env).returncode == 0
    for f in ("x.harc", "x.quality.hq"):                           # one byte changed inside each
        x = bytearray(orig[f])
        x[len(x) // 3] ^= 0x5A
        (tmp_path / f).write_bytes(bytes(x))
    damaged = {f: (tmp_path / f).read_bytes() for f in names}
    r = _harc(["-R", str(tmp_path / "x.harc"), "-n"], env)
    assert r.returncode == 1 and "[recovery] x.harc damaged: 1 of" in r.stdout and "[recovery] x.quality.hq damaged: 1 of" in r.stdout and "[recovery] x.id.hi ok" in r.stdout, r.stdout[-2000:]
    assert {f: (tmp_path / f).read_bytes() for f in names} == damaged
    r = _harc(["-R", str(tmp_path / "x.harc")], env)
    assert r.returncode == 0 and "[recovery] x.harc repaired: 1 of" in r.stdout and "[recovery] x.quality.hq repaired: 1 of" in r.stdout, r.stdout[-2000:]
    assert {f: (tmp_path / f).read_bytes() for f in names} == orig
    r = _harc(["-d", str(tmp_path / "x.harc"), "-p", "-q"], env)
    assert r.returncode == 0, r.stdout[-2000:]
    assert (tmp_path / "x.d.fastq").read_bytes() == fastq
