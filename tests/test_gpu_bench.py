"""bench.py on the GPU: a plain run prints the headline line and runs nothing the headline does not need; --dump-outputs writes the streams of
the last timed step, the same for the same inputs whatever the number of steps and the same as the library returns; --full adds the round trip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "mini"] + args, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout                                  # ONE line on stdout
    return json.loads(lines[0])


def _dump(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_and_dump_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", a])
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0, d
    assert d["unit"] == "Mreads/s" and d["higher_is_better"] is True and d["metric"] and d["dtype"]
    for leg in ("roundtrip", "cpu_baseline", "exact_mode", "size_vs_reference_t8", "other_configs", "end_to_end"):
        assert leg not in d, leg
    _bench(["--steps", "1", "--warmup", "0", "--dump-outputs", b])
    da, db = _dump(a), _dump(b)
    assert set(da) == set(db) and "streams.npy" in da and "S2_SEQ_0.npy" in da and "S2_ORDER.npy" in da
    rows = da["streams.npy"]
    assert rows.ndim == 2 and rows.shape[1] == 2 and rows[:, 0].sum() > 0
    assert len(da) - 1 == int((rows[:, 0] > 0).sum())                 # one file per stream that is not empty
    assert sum(os.path.getsize(os.path.join(a, f)) for f in da) <= 64 << 20
    for f in da:
        assert da[f].dtype in (np.float32, np.float64) and da[f].size > 0, f
        assert np.array_equal(da[f], db[f]), f

    # the same inputs through a context of this process: every row of streams.npy is the length and crc32 of the stream the library returns, and
    # every file holds that stream's elements at the positions the documented sampling rule picks
    import zlib
    import torch
    import bench
    import harc_amd
    n, L, G, err, _ = bench.WORKLOADS["mini"]
    names = bench.dump_stream_names(8, False)
    assert rows.shape[0] == len(names)
    per = min(1 << 17, (48 << 20) // (8 * len(names)))
    h = harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=8, device=0, profile=1))
    try:
        bench.install_synthetic(h, n, L, G, err, 1000, torch.device("cuda", 0), bench.SPIKES.get("mini"), signature=False)
        h.reorder(); h.encode()
        for (sid, e, stem), (ln, crc) in zip(names, rows):
            want = h.stream(sid, e)
            assert ln == len(want) and crc == zlib.crc32(want), stem
            if not want:
                assert stem + ".npy" not in da, stem
                continue
            u32 = sid in ("S2_ORDER", "S2_ORDER_N_PE")
            v = np.frombuffer(want, np.uint32 if u32 else np.uint8)
            if v.shape[0] > per:
                stride = v.shape[0] // per
                v = v[np.arange(per) * stride + np.random.default_rng(zlib.crc32(stem.encode())).integers(0, stride, per)]
            got = da[stem + ".npy"]
            assert got.dtype == (np.float64 if u32 else np.float32) and np.array_equal(got, v.astype(got.dtype)), stem
    finally:
        h.close()


def test_full_adds_the_round_trip():
    d = _bench(["--steps", "1", "--warmup", "1", "--full", "--no-cpu"])
    assert d["steps"] == 1 and d["roundtrip"]["ok"] and d["roundtrip"]["reads_decoded"] == 200_000, d["roundtrip"]
