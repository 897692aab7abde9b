"""The prior allele-frequency estimate of call-exact (--estimate-prior-frequencies) at BASELINE configs[3] -- hexaploid, 16
haplotypes x 10 SNVs, 500 reads, 256 units (256 records of one sample) -- on one GPU: ms of the one likelihood pass (llks64 alone),
ms per iteration of the resident path (counts + update launches over the stored likelihoods) and of the recompute path (the
streaming form's two passes over the reads for `freqs`, as the fallback runs it without the joint values kept, and with them kept
for comparison), the resident iteration's achieved bytes per second against U * G * 8 per pass over the array, and the largest
deviation between the two paths' first iteration.  HIP events; every figure the median of `reps` windows after a warm-up, the two
paths alternating within one process.  One JSON line.    python tools/estimate_once.py [units] [reps] [iterations per window]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd.device import ExactDeviceBatch, ExactFrequencyEstimate
from mchap_amd.synth import synth_units

U = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
per = int(sys.argv[3]) if len(sys.argv) > 3 else 50
K, H, M, R, F = 6, 16, 10, 500, 0.1
rng = np.random.default_rng(4)
reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, window=(5, 10), first_unit=400)
haps = np.unique(rng.integers(0, 2, size=(64, M)).astype(np.int8), axis=0)[:H]
f0 = np.full((U, H), 1.0 / H)


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


def estimate():
    est = ExactFrequencyEstimate(np.full(U, H, dtype=np.int32), f0, 1, K)
    est.add_group(llks, H, K, np.full(U, F), np.arange(U), np.zeros(U, dtype=np.int64))
    return est


est = estimate()
recompute = ExactDeviceBatch(reads, K, haps, None, (F, f0), cache_joint=False)
cached = ExactDeviceBatch(reads, K, haps, None, (F, f0), cache_joint=True)
freqs_only = dict(freqs=(U * H, torch.float64))
res = {"units": U, "genotypes": plain.G, "reads": R, "reps": reps, "iterations_per_window": per}
# the first iteration of both paths from the same f_0
est.step(0.0, 1 << 30)
first = est.results()[0]
dev = float(np.max(np.abs(first - recompute.run_freqs(f0))))
res["first_iteration_max_deviation"] = dev
windows = {}
for name, fn, n in (("likelihood_pass_ms", plain.run_llks64, 1), ("resident_iteration_ms", lambda: est.step(0.0, 1 << 30), per),
                    ("recompute_iteration_ms", lambda: recompute._run_only(**freqs_only), 3),
                    ("recompute_iteration_joint_kept_ms", lambda: cached._run_only(**freqs_only), 3)):
    windows[name] = timed(fn, n)
# ... and once more in the other order: the spread between the two orders is the noise of the session
for name, fn, n in (("recompute_iteration_ms", lambda: recompute._run_only(**freqs_only), 3),
                    ("resident_iteration_ms", lambda: est.step(0.0, 1 << 30), per)):
    again = timed(fn, n)
    res[name + "_second_window"] = again[0]
for name, (med, lo, hi) in windows.items():
    res[name] = med
    res[name + "_range"] = [lo, hi]
ms = res["resident_iteration_ms"]
res["resident_bytes_per_pass"] = U * plain.G * 8
res["resident_achieved_GB_per_s"] = U * plain.G * 8 / (ms * 1e-3) / 1e9
res["recompute_over_resident"] = res["recompute_iteration_ms"] / ms
print(json.dumps(res))
