"""GPU: results do not depend on how the units are sharded over ranks, and bench.py's N > 1 path runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shards_reproduce_the_unsharded_batch():
    """Rank r owns a contiguous block of units and keys every unit's RNG streams by its global id
    (mchap_amd/shard.py, DenovoDeviceBatch(first_stream=...)): two half batches == one full batch, bit for bit."""
    from mchap_amd import DenovoMCMC
    from mchap_amd.device import DenovoDeviceBatch
    from mchap_amd.shard import shard_range
    from mchap_amd.synth import synth_units

    n = 7
    reads, _, _ = synth_units(n, n_pos=6, n_reads=60, window=(3, 6))
    model = DenovoMCMC(ploidy=4, n_alleles=[2] * 6, steps=150, chains=2, random_seed=3)
    full = DenovoDeviceBatch(model, reads)
    full.run()
    full.posterior(50)
    w_full, fixed_full, llk_full, _ = full.traces()
    post_full = full.posterior_host()
    for rank in range(2):
        a, b = shard_range(n, rank, 2)
        part = DenovoDeviceBatch(model, reads[a:b], first_stream=a)
        part.run()
        part.posterior(50)
        w, fixed, llk, _ = part.traces()
        assert np.array_equal(w, w_full[a:b]) and np.array_equal(fixed, fixed_full[a:b])
        assert np.array_equal(llk, llk_full[a:b])
        post = part.posterior_host()
        assert np.array_equal(post["mode"], post_full["mode"][a:b])
        assert np.array_equal(post["stats"], post_full["stats"][a:b])


def test_bench_two_ranks_on_one_gpu():
    """bench.py under torch.distributed.run with two ranks (gloo rendezvous: RCCL refuses two ranks on one device);
    the line must report the whole job."""
    env = dict(os.environ, MCHAP_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--loci", "512", "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert abs(d["value"] - 2 * 512 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["roofline"]["kernel"].startswith("denovo_")
    # the posterior records of both ranks were all-gathered inside the timed region and rank 0 verified the other
    # rank's records against its own run of those units
    assert d["gather_ms"] is not None and d["gather_ms"] >= 0 and d["gather_checked_units"] == 8


def test_bench_strong_scaling_uneven_shards():
    """--total-loci: BASELINE.json configs[2]'s mode (a fixed number of loci sharded over the ranks), uneven split."""
    env = dict(os.environ, MCHAP_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29534", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--total-loci", "777", "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["scaling"] == "strong" and d["n_gpus"] == 2
    assert abs(d["value"] - 777 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["gather_checked_units"] == 8


def test_bench_gpus_flag_starts_the_ranks_itself():
    """`python bench.py --gpus 2` with no launcher around it: the parent starts two fresh rank processes before anything touches
    the GPU and relays rank 0's line (round 3's flag was parsed and ignored: one rank, n_gpus 1).  On a box with fewer GPUs than
    ranks the ranks share the device and gloo carries the gather; with a GPU each it is RCCL -- the line says which."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MCHAP_BENCH_BACKEND")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--loci", "512", "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["world_size"] == 2 and d["config"]["backend"] in ("nccl", "gloo")
    assert abs(d["value"] - 2 * 512 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["gather_checked_units"] == 8
    # a launcher that started a different number of ranks than --gpus says is an error, not a silent single-rank run
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0", "--loci", "64",
                          "--no-cpu-baseline", "--no-extras"], env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert bad.returncode != 0 and "--gpus 4" in bad.stderr


def test_bench_single_rank_over_rccl():
    """The RCCL calls of the N > 1 path on the one GPU there is (VERDICT r4 #5a): `bench.py --gpus 1` with MCHAP_BENCH_DIST=1 joins a
    process group of one rank on the **nccl** backend (= RCCL on ROCm) -- RCCL initialisation with GPU_MAX_HW_QUEUES=16 in the rank,
    the all_gather of device-resident record tensors issued from the four side streams of the passes in flight,
    barrier(device_ids=...), the all_reduce of the timing -- everything a rank of an 8-GPU run does but the xGMI transfers."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MCHAP_BENCH_BACKEND")}
    env.update(MCHAP_BENCH_DIST="1", MCHAP_BENCH_BACKEND="nccl", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--loci", "1024", "--inflight", "4",
           "--no-cpu-baseline", "--no-extras", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["config"]["backend"] == "nccl" and d["config"]["world_size"] == 1
    assert d["gather_ms"] is not None and d["gather_ms"] >= 0
    assert abs(d["value"] - 1024 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]


def test_bench_config3_at_its_size_eight_ranks_on_one_gpu():
    """BASELINE.json configs[2] at its size (VERDICT r4 #5b): 100 000 loci sharded over EIGHT ranks (12 500 each; `--total-loci`), one
    pass, the ranks sharing the one device there is (gloo carries the gather), the cross-rank record check on."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MCHAP_BENCH_BACKEND")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--total-loci", "100000", "--inflight", "1", "--steps", "1",
           "--warmup", "0", "--no-cpu-baseline", "--no-extras", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1800, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 8 and d["scaling"] == "strong" and d["config"]["world_size"] == 8
    assert abs(d["value"] - 100000 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["gather_checked_units"] == 8
