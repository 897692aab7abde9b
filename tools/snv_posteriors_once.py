"""The SNV genotype posteriors of call-exact (--snv-calls) at the shape of tools/evidence_once.py -- hexaploid, 16 haplotypes, 500
reads, 256 units -- over 8 biallelic SNVs, on one GPU: ms of the one likelihood pass (llks64 alone), ms of the SNV launch over the
stored likelihoods (the evidence launches for the normaliser, the tiles, the combine), and for comparison ms of what gave the same
numbers before: the array form's posteriors [U][G] formed on the device and read back, then the marginalisation of the definition in
numpy on the host (application._snv_genotype_ranks and a bincount per unit and SNV; the genotype table and the ranks are computed
once, outside the timed part).  The values are checked against the host definition on the first unit.  HIP events for the device
figures, a wall clock for the baseline (it ends on the host); every figure the median of `reps` windows after a warm-up.  One JSON
line.
python tools/snv_posteriors_once.py [units] [reps] [launches per window]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import application
from mchap_amd.device import ExactDeviceBatch, ExactSnvPosteriors
from mchap_amd.synth import synth_units

U = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
per = int(sys.argv[3]) if len(sys.argv) > 3 else 20
K, H, M, R = 6, 16, 8, 500
F = 0.1
rng = np.random.default_rng(4)
reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, window=(5, 10), first_unit=400)
haps = np.unique(rng.integers(0, 2, size=(64, M)).astype(np.int8), axis=0)[:H]
haps[0] = 0   # (haplotype 0 is REF: allele 0 at every SNV)
f = rng.dirichlet(np.full(H, 2.0), size=U)


def timed(fn, n, wall=False):
    """Median ms per call of fn over `reps` windows of n calls (one warm-up window first); wall: time.perf_counter around
    synchronised calls instead of HIP events."""
    out = []
    for w in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if w:
            out.append(((t1 - t0) * 1e3 if wall else e0.elapsed_time(e1)) / n)
    return float(np.median(out)), float(min(out)), float(max(out))


plain = ExactDeviceBatch(reads, K, haps, None, None, cache_joint=False)
llks = plain.run_llks64()
torch.cuda.synchronize()
snv = ExactSnvPosteriors()
d_f = torch.from_numpy(f).to(snv.device)
rows = np.arange(U, dtype=np.int32)
alleles = np.broadcast_to(haps, (U, H, M))
launch = lambda: snv.add_group(llks, H, K, F, rows, d_f, alleles)

arrays = ExactDeviceBatch(reads, K, haps, None, (F, f), cache_joint=False)
table = application._genotype_table(H, K)
ranks = [application._snv_genotype_ranks(table, haps[:, j]) for j in range(M)]
S = K + 1


def baseline():
    """The array form's posteriors read back, then the numpy marginalisation per unit and SNV."""
    arrays.run(streaming=False, arrays=True)
    post = arrays.out["posteriors"].cpu().numpy().reshape(U, plain.G)
    out = np.empty((U, M, S))
    for u in range(U):
        for j in range(M):
            out[u, j] = np.bincount(ranks[j], weights=post[u], minlength=S)
    return out


res = {"units": U, "genotypes": plain.G, "reads": R, "snvs": M, "snv_genotypes": S, "inbreeding": F, "reps": reps,
       "launches_per_window": per}
got = launch().cpu().numpy()
want = application.snv_posterior_unit(llks[:plain.G].cpu().numpy(), H, K, F, f[0], haps)
res["unit0_max_deviation_from_host"] = float(np.max(np.abs(got[0] - want)))
res["baseline_max_deviation_from_launch"] = float(np.max(np.abs(baseline() - got)))   # (the array form rounds its likelihoods to float32)
windows = {}
for name, fn, n, wall in (("likelihood_pass_ms", plain.run_llks64, 1, False), ("snv_launch_ms", launch, per, False),
                          ("baseline_readback_numpy_ms", baseline, 1, True)):
    windows[name] = timed(fn, n, wall)
# ... and the launch once more after the baseline: the spread between the two windows is the noise of the session
res["snv_launch_ms_second_window"] = timed(launch, per)[0]
for name, (med, lo, hi) in windows.items():
    res[name] = med
    res[name + "_range"] = [lo, hi]
res["snv_bytes_read"] = 2 * U * plain.G * 8   # the likelihoods, once per pass
res["baseline_over_likelihood_plus_snv"] = res["baseline_readback_numpy_ms"] / (res["likelihood_pass_ms"] + res["snv_launch_ms"])
print(json.dumps(res))
