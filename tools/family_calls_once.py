"""The family calls of call-exact (--family-calls) on one GPU: tetraploid, 16 haplotypes, 500 reads -- G = 3876 genotypes, the
[G_P][G_Q] array of a record 120 MB --, records of two parents and six progeny.  Timed: ms of the one likelihood pass (llks64
alone), ms of the family launches over the stored likelihoods (mchap_exact_family_device: the parents' tables, the sum over the
progeny, the streaming pass, the back projection of every progeny) for all records in one call, and for comparison ms of the only
way to the same numbers before: llks64 read back, then application.family_unit in numpy -- whose dense products go through BLAS
-- for every record.  The baseline is timed over the first `baseline records` records, each by a wall clock, and scaled to the
batch.  The values are checked against the host definition on those records.  HIP events for the device figures, every one the
median of `reps` windows after a warm-up.  One JSON line.
python tools/family_calls_once.py [records] [reps] [launches per window] [baseline records] [progeny per record]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import application
from mchap_amd.device import ExactDeviceBatch, ExactFamily
from mchap_amd.synth import synth_units

NR = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
per = int(sys.argv[3]) if len(sys.argv) > 3 else 2
RB = min(NR, int(sys.argv[4])) if len(sys.argv) > 4 else min(NR, 2)
N = int(sys.argv[5]) if len(sys.argv) > 5 else 6
U = NR * (N + 2)
K, H, M, R = 4, 16, 8, 500
F, E = 0.1, (0.01, 0.01)
rng = np.random.default_rng(4)
reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, window=(5, 10), first_unit=400)
haps = np.unique(rng.integers(0, 2, size=(64, M)).astype(np.int8), axis=0)[:H]
haps[0] = 0   # (haplotype 0 is REF: allele 0 at every SNV)
f = rng.dirichlet(np.full(H, 2.0), size=NR)


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
G = batch.G
# the batch's units: the P of every record, then the Q of every record, then the progeny record by record
llk_p, llk_q, llk_c = llks[:NR * G], llks[NR * G:2 * NR * G], llks[2 * NR * G:]
fam = ExactFamily()
d_f = torch.from_numpy(f).to(fam.device)
state = {}


def launches():
    state["got"] = fam.call(llk_p, llk_q, llk_c, H, K, K, d_f, E, F, F)


def baseline():
    """llks64 read back, then the definition in numpy, record by record: (results, seconds of every record)."""
    t0 = time.perf_counter()
    host = llks.cpu().numpy().reshape(U, G)
    back = time.perf_counter() - t0
    out, secs = [], []
    for r in range(RB):
        t0 = time.perf_counter()
        out.append(application.family_unit(host[r], K, F, host[NR + r], K, F, H, f[r], E,
                                           [host[2 * NR + r * N + c] for c in range(N)]))
        secs.append(time.perf_counter() - t0)
    return out, secs, back


res = {"records": NR, "progeny_per_record": N, "units": U, "genotypes": G, "reads": R, "haplotypes": H, "inbreeding": F, "gamete_error": E[0],
       "reps": reps, "launches_per_window": per, "baseline_records": RB,
       "workspace_bytes": ExactFamily.workspace_bytes(NR, H, K, K)}
launches()
got = {k: v.cpu().numpy() for k, v in state["got"].items()}
want, secs, back = baseline()
res["baseline_readback_ms"] = back * 1e3
res["baseline_numpy_ms_per_record"] = float(np.median(secs)) * 1e3
res["baseline_numpy_ms_per_record_range"] = [min(secs) * 1e3, max(secs) * 1e3]
res["baseline_readback_numpy_ms_scaled_to_batch"] = back * 1e3 + res["baseline_numpy_ms_per_record"] * NR
res["max_deviation_of_parent_posterior_from_host"] = float(max(max(np.abs(got["post_p"][r] - want[r]["post_p"]).max(),
                                                                   np.abs(got["post_q"][r] - want[r]["post_q"]).max()) for r in range(RB)))
res["max_deviation_of_progeny_mode_probability_from_host"] = float(max(np.abs(got["prob_c"][r] - want[r]["probs"]).max() for r in range(RB)))
res["max_deviation_of_predictive_log_evidence_from_host"] = float(max(np.abs(got["pred"][r] - want[r]["pred"]).max() for r in range(RB)))
res["max_deviation_of_log_z_from_host"] = float(max(abs(got["log_z"][r] - want[r]["log_z"]) for r in range(RB)))
res["modes_equal_host"] = bool(all(int(got["mode_p"][r]) == want[r]["mode_p"] and int(got["mode_q"][r]) == want[r]["mode_q"] and
                                   np.array_equal(got["mode_c"][r], want[r]["modes"]) for r in range(RB)))
windows = {"likelihood_pass_ms": timed(batch.run_llks64, 1), "family_launches_ms": timed(launches, per)}
# ... and once more: the spread between the two windows is the noise of the session
res["family_launches_ms_second_window"] = timed(launches, per)[0]
for name, (med, lo, hi) in windows.items():
    res[name] = med
    res[name + "_range"] = [lo, hi]
res["baseline_over_likelihood_plus_family"] = res["baseline_readback_numpy_ms_scaled_to_batch"] / (res["likelihood_pass_ms"] + res["family_launches_ms"])
print(json.dumps(res))
