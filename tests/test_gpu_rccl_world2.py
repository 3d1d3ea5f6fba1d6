"""RCCL at world size 2 -- runs only where the box has at least two GPUs (the builders' boxes have one: there the suite reaches the library's
collectives over RCCL at world 1 and over the file transport at world 2 / 3, tests/test_gpu_multigpu.py and tests/test_gpu_replicate.py).
On the first multi-GPU box this file verifies, without anybody's help:

  * both multi-GPU modes through `bench.py --gpus 2` (one process per GPU, torch.distributed.run, RCCL over xGMI): the round trip holds
    (all-reduced signature of the decoded streams == all ranks' inputs), and the line reports two GPUs;
  * design (R) byte for byte: two ranks over RCCL -- all-gather of the reads, chains partitioned, one all-gather of the walked steps per
    super-round, stage II partitioned with ONE ncclAllReduce(min) of the claims -- assembled as harc_amd_merge_shard_files does == one GPU;
  * the bucket exchange (grouped ncclSend / ncclRecv to another peer): decodes to the input, ids global."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ngpu():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:  # pragma: no cover
        return 0


# HARC_TEST_RCCL_WORLD=1 rehearses the very same scripts at world size 1 on a one-GPU box (the builders did: the scripts themselves are sound)
WORLD = int(os.environ.get("HARC_TEST_RCCL_WORLD", "2"))
needs2 = pytest.mark.skipif(_ngpu() < WORLD, reason="needs two GPUs (RCCL refuses two ranks on one device)")


@needs2
@pytest.mark.parametrize("mode", ["bucket", "replicate"])
def test_bench_two_gpus_round_trip(mode):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(WORLD), "--workload", "c3m", "--steps", "2", "--warmup", "1", "--full", "--no-cpu", "--no-side-legs",
                        "--mg-mode", mode, "--launch-timeout", "600", "--watchdog", "240"] + (["--via-launcher", "--force-dist"] if WORLD == 1 else []), cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == WORLD and d["roundtrip"]["ok"] and d["roundtrip"]["reads_decoded"] == WORLD * 4_000_000, d["roundtrip"]
    assert d["value"] > 0


WORKER = textwrap.dedent("""
    import os, sys, numpy as np, torch, torch.distributed as dist
    sys.path.insert(0, %r)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", device_id=dev)
    import harc_amd
    from harc_amd import multigpu
    from tests import gen, shard_model
    from tests.test_gpu_replicate import _collect, _assemble
    L, E, K, S = 100, 4, 0, 16
    arr = gen.reads_array(606, 600000, L, 2400000, err=0.01)
    sl = shard_model.slices_of(arr, world)[rank]
    hasN = (sl == ord("N")).any(1)
    h = harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S, device=rank))
    assert multigpu.init_comm(h, dist, dev) == (world, rank)
    h.set_reads_ascii(shard_model.lines(sl[~hasN]), int((~hasN).sum()), L + 1)
    h.set_nreads_ascii(shard_model.lines(sl[hasN]), int(hasN.sum()), L + 1)
    mode = sys.argv[1]
    if mode == "replicate":
        info = h.replicate_exchange()
    else:
        info = h.shard_exchange()
    h.reorder(); h.encode()
    piece = dict(files=_collect(h, E), sig=h.decode_signature(), info=info)
    h.comm_barrier()
    h.close()
    pieces = [None] * world
    dist.gather_object(piece, pieces if rank == 0 else None, dst=0)
    if rank == 0:
        n = arr.shape[0]
        assert sum(p["sig"][0] for p in pieces) == n, [p["sig"] for p in pieces]
        if mode == "replicate":
            allN = (arr == ord("N")).any(1)
            one = harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S, device=0))
            one.set_reads_ascii(shard_model.lines(arr[~allN]), int((~allN).sum()), L + 1)
            one.set_nreads_ascii(shard_model.lines(arr[allN]), int(allN.sum()), L + 1)
            one.reorder(); one.encode()
            want = _collect(one, E)
            one.close()
            got = _assemble(pieces, E, L)
            bad = [k for k in want if got[k] != want[k]]
            assert not bad, bad
        else:
            # every read decoded exactly once, by the rank that owns its bucket: the signatures of the decoded shards add up to the inputs'
            tot = [0, 0, 0]
            for p in pieces:
                tot[0] += p["sig"][0]; tot[1] = (tot[1] + p["sig"][1]) %% (1 << 64); tot[2] ^= p["sig"][2]
            hh = harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=1, device=0))
            allN = (arr == ord("N")).any(1)
            hh.set_reads_ascii(shard_model.lines(arr[~allN]), int((~allN).sum()), L + 1)
            hh.set_nreads_ascii(shard_model.lines(arr[allN]), int(allN.sum()), L + 1)
            assert tuple(tot) == hh.input_signature()
            hh.close()
        print("WORLD2_OK")
    dist.barrier()
    dist.destroy_process_group()
""") % ROOT


@needs2
@pytest.mark.parametrize("mode", ["replicate", "bucket"])
def test_two_ranks_over_rccl(mode, tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", HARC_AMD_COMM_TIMEOUT="240")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(WORLD), "--master-addr", "127.0.0.1",
                          "--master-port", "29551", str(script), mode], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert out.returncode == 0 and "WORLD2_OK" in out.stdout, out.stdout[-4000:]


def test_skips_are_honest():
    """on a one-GPU box the tests above are skipped, not passed: this one says so in the report"""
    if _ngpu() < WORLD:
        pytest.skip("one GPU here: RCCL at world size 2 has not run (see the module docstring)")
