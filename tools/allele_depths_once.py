"""The expected allele depths of call-exact (--allele-depths) at the shape of tools/evidence_once.py -- hexaploid, 16 haplotypes, 500
reads, 256 units -- on one GPU: ms of the one likelihood pass (llks64 alone), ms of the support launches over the stored
likelihoods and the resident reads (the evidence launches for the normaliser, the tiles, the combine), and for comparison ms of
the only way to the same numbers before: llks64 and the read tensors read back, then application.allele_support_unit in numpy for
every unit.  The baseline is slow (the genotype table, the prior and the posterior of 54 264 genotypes per unit on the host), so it
is timed once, over the first `baseline units` units, by a wall clock, and reported per unit and scaled to the batch.  The values
are checked against the host definition on those units.  HIP events for the device figures, every one the median of `reps` windows
after a warm-up.  One JSON line.
python tools/allele_depths_once.py [units] [reps] [launches per window] [baseline units]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import _lib, application
from mchap_amd.device import ExactDeviceBatch, ExactReadSupport
from mchap_amd.synth import synth_units

U = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
per = int(sys.argv[3]) if len(sys.argv) > 3 else 10
UB = min(U, int(sys.argv[4])) if len(sys.argv) > 4 else U
K, H, M, R = 6, 16, 8, 500
F = 0.1
rng = np.random.default_rng(4)
reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, window=(5, 10), first_unit=400)
haps = np.unique(rng.integers(0, 2, size=(64, M)).astype(np.int8), axis=0)[:H]
haps[0] = 0   # (haplotype 0 is REF: allele 0 at every SNV)
f = rng.dirichlet(np.full(H, 2.0), size=U)


def timed(fn, n):
    """Median ms per call of fn over `reps` windows of n calls (one warm-up window first), by HIP events."""
    out = []
    for w in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if w:
            out.append(e0.elapsed_time(e1) / n)
    return float(np.median(out)), float(min(out)), float(max(out))


batch = ExactDeviceBatch(reads, K, haps, None, None, cache_joint=False)
llks = batch.run_llks64()
torch.cuda.synchronize()
support = ExactReadSupport()
d_f = torch.from_numpy(f).to(support.device)
rows = np.arange(U, dtype=np.int32)
launch = lambda: support.add_group(batch, llks, F, rows, d_f)


def baseline():
    """llks64 and the read tensors read back, then the definition in numpy, unit by unit."""
    host_llks = llks.cpu().numpy().reshape(U, batch.G)
    host_reads = batch.d_reads.cpu().numpy().reshape(U, R, M, reads.shape[3])
    return np.stack([application.allele_support_unit(host_reads[u], None, haps, host_llks[u], K, F, f[u])[0] for u in range(UB)])


res = {"units": U, "genotypes": batch.G, "reads": R, "haplotypes": H, "inbreeding": F, "reps": reps, "launches_per_window": per,
       "rows_per_tile": int(_lib.lib().mchap_exact_support_tile(R, H, K)), "baseline_units": UB}
got = launch().cpu().numpy()
t0 = time.perf_counter()
want = baseline()
res["baseline_readback_numpy_ms_per_unit"] = (time.perf_counter() - t0) * 1e3 / UB
res["baseline_readback_numpy_ms_scaled_to_batch"] = res["baseline_readback_numpy_ms_per_unit"] * U
res["max_deviation_from_host_over_read_weight"] = float(np.max(np.abs(got[:UB] - want))) / R
res["depth_sum_over_read_weight_range"] = [float(got.sum(axis=1).min()) / R, float(got.sum(axis=1).max()) / R]
host_llks = llks.cpu().numpy().reshape(U, batch.G)
res["genotypes_with_p_above_1e-300_median"] = float(np.median((host_llks > host_llks.max(axis=1, keepdims=True) - 690).sum(axis=1)))
windows = {}
for name, fn, n in (("likelihood_pass_ms", batch.run_llks64, 1), ("support_launch_ms", launch, per)):
    windows[name] = timed(fn, n)
# ... and the launch once more: the spread between the two windows is the noise of the session
res["support_launch_ms_second_window"] = timed(launch, per)[0]
for name, (med, lo, hi) in windows.items():
    res[name] = med
    res[name + "_range"] = [lo, hi]
res["baseline_over_likelihood_plus_support"] = res["baseline_readback_numpy_ms_scaled_to_batch"] / (res["likelihood_pass_ms"] + res["support_launch_ms"])
print(json.dumps(res))
