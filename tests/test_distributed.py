"""N > 1 path on CPU: two gloo ranks exercise the stream sharding and the reporting reductions
that bench.py uses with RCCL on the GPUs (no data-path collective exists)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from sdrdaemon_amd import sharding


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ids = sharding.stream_ids(rank, world, 8)
    # every rank "processes" its streams: elapsed differs per rank, samples = 8 streams x 1000
    elapsed, total = sharding.aggregate(0.5 + 0.25 * rank, len(ids) * 1000, dist)
    gathered = [None] * world
    dist.all_gather_object(gathered, ids)
    q.put((rank, ids, elapsed, total, gathered))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_and_aggregation():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res.sort()
    all_ids = res[0][1] + res[1][1]
    assert all_ids == list(range(16))  # disjoint cover: stream s on rank s // 8
    for rank, ids, elapsed, total, gathered in res:
        assert all(sharding.owner(i, 8) == rank for i in ids)
        assert elapsed == pytest.approx(0.75)  # MAX over ranks
        assert total == 16000.0  # SUM over ranks
        assert gathered == [res[0][1], res[1][1]]


def test_single_process_passthrough():
    assert sharding.aggregate(1.5, 10) == (1.5, 10.0)
    assert sharding.stream_ids(3, 8, 8) == list(range(24, 32))
    with pytest.raises(ValueError):
        sharding.stream_ids(8, 8, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("extra,scaling,total", [([], "strong", 64), (["--streams", "0"], "weak", 16), (["--streams", "6"], "strong", 6)])
def test_bench_two_ranks_execute_on_one_gpu(extra, scaling, total):
    """The N > 1 branch of bench.py end to end (device selection, process group, barriers, sharded streams,
    aggregate()) under torch.distributed.run: two ranks share GPU 0 and use gloo for the two reporting reductions
    (--backend gloo; the driver's 8-GPU run uses nccl = RCCL).  That is all one GPU can show of the N > 1 path."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "3",
           "--warmup", "1", "--cpu-seconds", "0", "--preroll-seconds", "0.05", "--log2-samples", "22"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2 and res["scaling"] == scaling and res["steps"] == 3
    ids = res["config"]["stream_ids_by_rank"]
    assert len(ids) == 2 and sorted(ids[0] + ids[1]) == list(range(total))  # disjoint cover of the job's streams
    assert not set(ids[0]) & set(ids[1])
    n = 1 << 22
    # value = all ranks' samples / the slowest rank's time
    assert res["value"] == pytest.approx(total * n * 3 / (res["ms_per_step"] * 3e-3) / 1e6, rel=1e-3)
    assert res["value"] > 1000.0


@pytest.mark.gpu
def test_bench_executes_the_rccl_branch_on_one_gpu():
    """bench.py --force-dist: a world of ONE rank through init_process_group("nccl", device_id=...), two barriers and the two
    device-tensor all_reduce calls of sharding.aggregate(): the RCCL code path of the driver's 8-GPU run, executed.
    What it cannot show: more than one GPU -- unmeasured on multi-GPU hardware until a SCALE_r*.json exists."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--force-dist", "--backend", "nccl", "--steps", "3", "--warmup", "1",
           "--cpu-seconds", "0", "--preroll-seconds", "0.05", "--log2-samples", "22", "--no-configs", "--no-verify"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 1 and res["collectives"].startswith("nccl")
    assert res["value"] == pytest.approx(8 * (1 << 22) * 3 / (res["ms_per_step"] * 3e-3) / 1e6, rel=1e-3)


@pytest.mark.gpu
def test_bench_gpus_2_as_a_plain_process():
    """`python bench.py --gpus 2 ...` with NO launcher around it and WORLD_SIZE unset (the way the driver starts the 1-GPU run,
    VERDICT r3 #2): bench.py re-executes itself under torch.distributed.run; default layout for N > 1 = SURVEY 8e's fixed bank of
    64 streams, stream s on rank s mod G.  Two ranks share GPU 0 here (--backend gloo; nccl needs two GPUs)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SDRHIP_BENCH_STREAMS")}
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1",
           "--cpu-seconds", "0", "--preroll-seconds", "0.05", "--log2-samples", "21", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 2 and res["scaling"] == "strong" and res["config"]["streams_total"] == 64
    ids = res["config"]["stream_ids_by_rank"]
    assert ids[0] == list(range(0, 64, 2)) and ids[1] == list(range(1, 64, 2))
    assert res["verified"]["ok"] is True


@pytest.mark.gpu
def test_bench_n1_names_the_same_64_streams_as_n2():
    """One layout across N: the N = 1 run carries the job of N = 2 / 4 / 8 -- SURVEY 8e's bank of 64 streams -- as
    a `configs` line with the same stream ids that `--gpus 2` deals s mod 2 (test_bench_gpus_2_as_a_plain_process), verified like
    the headline; with SDRHIP_BENCH_SCALE=1 (a scaling sweep) that job IS the N = 1 headline."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SDRHIP_BENCH_STREAMS", "SDRHIP_BENCH_SCALE")}
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0",
            "--preroll-seconds", "0.05", "--log2-samples", "22", "--full"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["scaling"] == "weak" and res["config"]["layout"].startswith("weak") and res["config"]["stream_ids_by_rank"] == [list(range(8))]
    line = res["configs"][-1]
    assert line["layout"] == "strong" and line["streams_total"] == 64 and line["stream_ids"] == list(range(64))
    n2 = [list(range(0, 64, 2)), list(range(1, 64, 2))]  # what --gpus 2 deals (asserted on the real run in the test above)
    assert sorted(n2[0] + n2[1]) == line["stream_ids"]
    assert line["verified"]["ok"] is True and "headline_golden.json" in line["verified"]["against"]  # (64 x 2^22: the committed bank64 digests)
    assert all(c["verified"]["ok"] is True for c in res["configs"]), [c["config"][:40] for c in res["configs"] if not c["verified"]["ok"]]
    assert res["box"] is None or res["box"]["power_w"] > 0
    r = subprocess.run(base + ["--no-configs"], capture_output=True, text=True, timeout=900, cwd=root, env=dict(env, SDRHIP_BENCH_SCALE="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 1 and res["scaling"] == "strong" and res["config"]["streams_total"] == 64
    assert res["config"]["stream_ids_by_rank"] == [list(range(64))] and res["verified"]["ok"] is True


@pytest.mark.gpu
def test_bench_plain_run_carries_the_headline_alone():
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the headline figure and nothing that takes runs of its own
    (no output check, no power / clock sample, no `configs` lines, no CPU baselines: --full, tested above)"""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SDRHIP_BENCH_STREAMS", "SDRHIP_BENCH_SCALE")}
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--preroll-seconds", "0.05",
           "--log2-samples", "22"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["higher_is_better"] is True and res["unit"] == "Msamples/s" and res["dtype"] == "int32" and res["steps"] == 3
    assert res["value"] == pytest.approx(8 * (1 << 22) * 3 / (res["ms_per_step"] * 3e-3) / 1e6, rel=1e-3)
    assert res["roofline"]["launches"] > 0 and res["roofline"]["avg_launch_ms"] > 0
    assert res["verified"] is None and res["box"] is None
    assert not {"configs", "cpu_baseline", "gpu_over_cpu_1core", "cpu_baseline_all_cores"} & set(res)


def test_bench_gpus_n_without_enough_gpus_refuses_cleanly():
    """nccl with fewer visible GPUs than ranks: a message and exit code 2, not an assertion from inside torch (CPU box: 0 GPUs)"""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "64"], capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert r.returncode == 2 and "--backend gloo" in r.stderr
