"""The selfing rows of call-exact (--parentage --parentage-selfings) on one GPU: tetraploid and hexaploid, 16 haplotypes, 500
reads, 32 records of 16 candidates and 64 progeny each.  Timed: ms of the one likelihood pass (llks64 alone), ms of the candidates'
gamete launch, ms of the selfing-prior launch over the same stored likelihoods (its own gamete launch at a gamete error of 0
included), ms of the one selfing-evidence launch over all candidates and progeny.  For comparison the only way to the same
numbers without these launches: for the prior, the posteriors read back and application.selfing_prior in numpy, timed over the
first `baseline units` units and scaled to all; for the evidence, one ExactCross.posteriors launch per candidate over the log of
its selfing prior.  The values are checked against the host definition on the first `baseline units` units and the first record's
first two progeny.  HIP events (the host clock for numpy), every figure the median of `reps` windows after a warm-up.  One JSON
line per ploidy.
python tools/selfing_once.py [records] [reps] [launches per window] [baseline units] [ploidy ...]"""
import json
import os
import sys
import time
from math import comb

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import application
from mchap_amd.device import ExactCross, ExactDeviceBatch, ExactSelfing
from mchap_amd.synth import synth_units

NR = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
per = int(sys.argv[3]) if len(sys.argv) > 3 else 3
NB = int(sys.argv[4]) if len(sys.argv) > 4 else 2
ploidies = [int(x) for x in sys.argv[5:]] or [4, 6]
NC, NP = 16, 64          # candidates and progeny a record
H, M, R = 16, 8, 500
F, E = 0.1, 0.01


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


def once(K):
    t = K // 2
    U = NR * (NC + NP)
    rng = np.random.default_rng(4)
    reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, window=(5, 10), first_unit=400)
    haps = np.unique(rng.integers(0, 2, size=(64, M)).astype(np.int8), axis=0)[:H]
    haps[0] = 0   # (haplotype 0 is REF: allele 0 at every SNV)
    f = rng.dirichlet(np.full(H, 2.0), size=NR)
    batch = ExactDeviceBatch(reads, K, haps, None, None, cache_joint=False)
    llks = batch.run_llks64()
    torch.cuda.synchronize()
    G, NA = batch.G, comb(H + t - 1, t)
    # the batch's units: the candidates record by record, then the progeny record by record
    llk_cand, llk_c = llks[:NR * NC * G], llks[NR * NC * G:]
    dev, cross = ExactSelfing(), ExactCross()
    d_f = torch.from_numpy(f).to(dev.device)
    cand_rows = np.repeat(np.arange(NR, dtype=np.int32), NC)
    prog_rows = np.repeat(np.arange(NR, dtype=np.int32), NP)
    state = {}

    def gametes():
        state["gam"] = cross.gametes(llk_cand, H, K, F, cand_rows, d_f, E)

    def prior():
        state["log_s"], state["s"], _ = dev.selfing_prior(llk_cand, H, K, F, cand_rows, d_f, E)

    def evidence():
        state["z"] = dev.log_evidence(state["s"].view(NR, NC, G), llk_c, H, K)

    def baseline_evidence():
        """One posteriors launch per candidate over the log of its selfing prior."""
        log_s = state["log_s"].view(NR, NC, G)
        state["zb"] = [cross.posteriors(llk_c, H, K, log_s[:, i].contiguous(), prog_rows)[0] for i in range(NC)]

    def baseline_prior():
        """The first NB units on the host: the likelihoods read back, the posterior and selfing_prior in numpy."""
        host = llk_cand[:NB * G].cpu().numpy().reshape(NB, G)
        state["sb"] = [application.selfing_prior_unit(host[u], K, F, H, f[cand_rows[u]], E)["S"] for u in range(NB)]

    gametes(), prior(), evidence(), baseline_evidence()
    res = {"ploidy": K, "records": NR, "candidates": NC, "progeny": NP, "units": U, "genotypes": G, "gametes": NA, "reads": R, "haplotypes": H,
           "inbreeding": F, "gamete_error": E, "reps": reps, "launches_per_window": per, "baseline_units": NB,
           "prior_workspace_bytes": dev.prior_workspace_bytes(NR * NC, H, K), "evidence_workspace_bytes": dev.evidence_workspace_bytes(NR, NP, NC, H, K)}
    t0 = time.perf_counter()
    baseline_prior()
    res["baseline_prior_ms_per_unit"] = (time.perf_counter() - t0) * 1e3 / NB
    s = state["s"].cpu().numpy()
    res["max_deviation_of_the_prior_from_the_host_definition"] = float(max(np.max(np.abs(s[u] - state["sb"][u])) for u in range(NB)))
    z = state["z"].cpu().numpy()
    host_c = llk_c[:2 * G].cpu().numpy().reshape(2, G)
    want = np.stack([application.selfing_evidence(s[:NC], host_c[c]) for c in range(2)])
    res["max_deviation_of_the_evidence_from_the_host_definition"] = float(np.max(np.abs(z[0, :2] - want)))
    res["max_deviation_of_the_baseline_launches_from_the_evidence_launch"] = float(max(
        np.max(np.abs(got.cpu().numpy().reshape(NR, NP) - z[:, :, i])) for i, got in enumerate(state["zb"])))
    windows = {}
    for name, fn, k in (("likelihood_pass_ms", batch.run_llks64, 1), ("gamete_launch_ms", gametes, per), ("selfing_prior_launch_ms", prior, per),
                        ("selfing_evidence_launch_ms", evidence, per), ("baseline_evidence_ms", baseline_evidence, 1)):
        windows[name] = timed(fn, k)
    res["selfing_prior_launch_ms_second_window"] = timed(prior, per)[0]
    for name, (med, lo, hi) in windows.items():
        res[name] = med
        res[name + "_range"] = [lo, hi]
    res["baseline_prior_ms_scaled_to_all_units"] = res["baseline_prior_ms_per_unit"] * NR * NC
    res["baseline_prior_over_selfing_prior_launch"] = res["baseline_prior_ms_scaled_to_all_units"] / res["selfing_prior_launch_ms"]
    res["baseline_evidence_over_selfing_evidence_launch"] = res["baseline_evidence_ms"] / res["selfing_evidence_launch_ms"]
    return res


for K in ploidies:
    print(json.dumps(once(K)), flush=True)
