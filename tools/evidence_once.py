"""The model evidence of call-exact (--model-evidence) at BASELINE configs[3] -- hexaploid, 16 haplotypes x 10 SNVs, 500 reads, 256
units -- with a grid of 8 inbreeding values per unit, on one GPU: ms of the one likelihood pass (llks64 alone), ms of the evidence
launch over the stored likelihoods (all 8 grid points: tiles + combine), and for comparison ms of what the same numbers cost without
it: one streaming posterior pass per grid point under that prior (ExactDeviceBatch.run_freqs, whose first pass forms the
normaliser and drops it), 8 of them, each batch with its own F.  The streaming form does not return its normaliser, so the values
are checked against the host definition (application._host_log_prior) on the first unit.  HIP events; every figure the median of `reps` windows after a warm-up,
the evidence launch and the passes alternating within one process.  One JSON line.
python tools/evidence_once.py [units] [reps] [launches per window]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import application
from mchap_amd.device import ExactDeviceBatch, ExactModelEvidence
from mchap_amd.synth import synth_units

U = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
per = int(sys.argv[3]) if len(sys.argv) > 3 else 20
K, H, M, R = 6, 16, 10, 500
GRID = (0.0, 0.01, 0.05, 0.1, 0.2, 0.3, 0.5, 0.8)
rng = np.random.default_rng(4)
reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, window=(5, 10), first_unit=400)
haps = np.unique(rng.integers(0, 2, size=(64, M)).astype(np.int8), axis=0)[:H]
f = rng.dirichlet(np.full(H, 2.0), size=U)


def timed(fn, n):
    """Median ms per call of fn over `reps` windows of n calls (one warm-up window first)."""
    out = []
    for w in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if w:
            out.append(e0.elapsed_time(e1) / n)
    return float(np.median(out)), float(min(out)), float(max(out))


plain = ExactDeviceBatch(reads, K, haps, None, None, cache_joint=False)
llks = plain.run_llks64()
torch.cuda.synchronize()
ev = ExactModelEvidence()
grid = np.broadcast_to(np.array(GRID), (U, len(GRID)))
rows = np.arange(U)
d_f = torch.from_numpy(f).to(ev.device)
d_rows = torch.from_numpy(rows.astype(np.int32)).to(ev.device)
evidence = lambda: ev.add_group(llks, H, K, grid, d_rows, d_f)
streaming = [ExactDeviceBatch(reads, K, haps, None, (F, f), cache_joint=False) for F in GRID]   # one batch per grid point, its own prior


def passes():
    """One streaming posterior pass per grid point, each under its own prior, results read back (run_freqs)."""
    for batch in streaming:
        batch.run_freqs()


res = {"units": U, "genotypes": plain.G, "reads": R, "grid": list(GRID), "reps": reps, "launches_per_window": per}
got = evidence().cpu().numpy()
llk0 = llks[:plain.G].cpu().numpy()
table = application._genotype_table(H, K)
want = [application._logsumexp(llk0 + application._host_log_prior(table, H, K, F, f[0])) for F in GRID]
res["unit0_max_deviation_from_host"] = float(np.max(np.abs(got[0] - np.array(want))))
windows = {}
for name, fn, n in (("likelihood_pass_ms", plain.run_llks64, 1), ("evidence_launch_ms", evidence, per), ("streaming_passes_ms", passes, 1)):
    windows[name] = timed(fn, n)
# ... and once more in the other order: the spread between the two orders is the noise of the session
for name, fn, n in (("streaming_passes_ms", passes, 1), ("evidence_launch_ms", evidence, per)):
    res[name + "_second_window"] = timed(fn, n)[0]
for name, (med, lo, hi) in windows.items():
    res[name] = med
    res[name + "_range"] = [lo, hi]
res["evidence_bytes_read"] = U * plain.G * 8
res["evidence_achieved_GB_per_s"] = U * plain.G * 8 / (res["evidence_launch_ms"] * 1e-3) / 1e9
res["streaming_over_likelihood_plus_evidence"] = res["streaming_passes_ms"] / (res["likelihood_pass_ms"] + res["evidence_launch_ms"])
print(json.dumps(res))
