"""The cross calls of call-exact (--cross-calls) at the shape of tools/evidence_once.py -- hexaploid, 16 haplotypes, 500 reads, 256
units -- on one GPU.  The units are records of `units per record` samples each: two parents and their progeny.  Timed: ms of the
one likelihood pass (llks64 alone), ms of the three cross launches over the stored likelihoods (the parents' gamete tables after
their evidence launches, the records' cross priors, the progeny's posteriors with their own evidence launches), each on its own
and together, and for comparison ms of the only way to the same numbers before: llks64 read back, then
application.cross_prior_unit and cross_posterior in numpy for every record.  The baseline is timed once, over the first `baseline
records` records, by a wall clock, and scaled to the batch.  The values are checked against the host definition on those records.
HIP events for the device figures, every one the median of `reps` windows after a warm-up.  One JSON line.
python tools/cross_calls_once.py [units] [reps] [launches per window] [baseline records] [units per record]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import application
from mchap_amd.device import ExactCross, ExactDeviceBatch
from mchap_amd.synth import synth_units

U = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
per = int(sys.argv[3]) if len(sys.argv) > 3 else 10
S = int(sys.argv[5]) if len(sys.argv) > 5 else 8
NR = U // S                      # records
RB = min(NR, int(sys.argv[4])) if len(sys.argv) > 4 else min(NR, 2)
U = NR * S
K, H, M, R = 6, 16, 8, 500
F, E = 0.1, 0.01
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
cross = ExactCross()
d_f = torch.from_numpy(f).to(cross.device)
rows = np.arange(NR, dtype=np.int32)
crows = np.repeat(rows, S - 2)
state = {}


def gametes():
    state["p"] = cross.gametes(llk_p, H, K, F, rows, d_f, E)
    state["q"] = cross.gametes(llk_q, H, K, F, rows, d_f, E)


def prior():
    state["x"] = cross.cross_prior(state["p"], state["q"], H, K, K)


def posteriors():
    state["post"] = cross.posteriors(llk_c, H, K, state["x"], crows, F, d_f)


def launches():
    gametes(), prior(), posteriors()


def baseline():
    """llks64 read back, then the definition in numpy, record by record."""
    host = llks.cpu().numpy().reshape(U, G)
    out = []
    for r in range(RB):
        unit = application.cross_prior_unit(host[r], K, F, host[NR + r], K, F, H, f[r], (E, E))
        for c in range(S - 2):
            llk = host[2 * NR + r * (S - 2) + c]
            _, lz, mode, prob = application.cross_posterior(llk, unit["log_x"])
            out.append((lz - application._unit_posterior(llk, H, K, F, f[r])[1], mode, prob))
    return out


res = {"units": U, "records": NR, "units_per_record": S, "genotypes": G, "reads": R, "haplotypes": H, "inbreeding": F, "gamete_error": E,
       "reps": reps, "launches_per_window": per, "baseline_records": RB}
launches()
log_z, mode, prob, norm = (t.cpu().numpy() for t in state["post"])
t0 = time.perf_counter()
want = baseline()
res["baseline_readback_numpy_ms_per_record"] = (time.perf_counter() - t0) * 1e3 / RB
res["baseline_readback_numpy_ms_scaled_to_batch"] = res["baseline_readback_numpy_ms_per_record"] * NR
n = len(want)
res["max_deviation_of_log_bayes_factor_from_host"] = float(max(abs((log_z[i] - norm[i]) - want[i][0]) for i in range(n)))
res["max_deviation_of_mode_probability_from_host"] = float(max(abs(prob[i] - want[i][2]) for i in range(n)))
res["modes_equal_host"] = bool(all(int(mode[i]) == want[i][1] for i in range(n)))
windows = {}
for name, fn, k in (("likelihood_pass_ms", batch.run_llks64, 1), ("gamete_launches_ms", gametes, per), ("cross_prior_launch_ms", prior, per),
                    ("posterior_launches_ms", posteriors, per), ("cross_launches_ms", launches, per)):
    windows[name] = timed(fn, k)
# ... and the three once more: the spread between the two windows is the noise of the session
res["cross_launches_ms_second_window"] = timed(launches, per)[0]
for name, (med, lo, hi) in windows.items():
    res[name] = med
    res[name + "_range"] = [lo, hi]
res["baseline_over_likelihood_plus_cross"] = res["baseline_readback_numpy_ms_scaled_to_batch"] / (res["likelihood_pass_ms"] + res["cross_launches_ms"])
print(json.dumps(res))
