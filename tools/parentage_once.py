"""The parentage evidence of call-exact (--parentage) on one GPU: tetraploid and hexaploid, 16 haplotypes, 500 reads, 32 records
of 16 candidates and 64 progeny each.  Timed: ms of the one likelihood pass (llks64 alone), ms of the candidates' gamete launch,
ms of the population's row and the table, ms of the one parentage launch over the stored gamete tables and likelihoods -- all
17 x 17 pairs of rows (the candidates and the unknown parent) for every progeny --, and for comparison ms of the way to the same
numbers without it: one cross_prior and one posteriors launch (device.ExactCross) per pair over the same stored tables and
likelihoods, timed over the first `baseline pairs` pairs and scaled to the 136 hypotheses with a candidate in them (120 pairs and
16 candidates with an unknown parent).  The values are checked against the host definition (application.parentage_unit) on the
first record's first two progeny, and the timed pairs against the parentage launch's own entries.  HIP events, every figure the
median of `reps` windows after a warm-up.  One JSON line per ploidy.
python tools/parentage_once.py [records] [reps] [launches per window] [baseline pairs] [ploidy ...]"""
import json
import os
import sys
from math import comb

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import application
from mchap_amd.device import ExactDeviceBatch, ExactParentage
from mchap_amd.synth import synth_units

NR = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
per = int(sys.argv[3]) if len(sys.argv) > 3 else 3
NB = int(sys.argv[4]) if len(sys.argv) > 4 else 6
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
    par = ExactParentage()
    d_f = torch.from_numpy(f).to(par.device)
    cand_rows = np.repeat(np.arange(NR, dtype=np.int32), NC)
    prog_rows = np.repeat(np.arange(NR, dtype=np.int32), NP)
    state = {}

    def gametes():
        state["gam"] = par.gametes(llk_cand, H, K, F, cand_rows, d_f, E).view(NR, NC, NA)

    def table():
        state["table"] = par.table(state["gam"], d_f, H, t)

    def parentage():
        state["z"] = par.log_evidence(state["table"], state["table"], llk_c, H, t, t)

    def pair(i, j):
        """The same entry on the path without the parentage kernel: the pair's cross prior, then the progeny's posterior launch."""
        tab = state["table"]
        log_x = par.cross.cross_prior(tab[:, i].contiguous(), tab[:, j].contiguous(), H, K, K)
        return par.cross.posteriors(llk_c, H, K, log_x, prog_rows)[0]

    pairs = [(i, j) for i in range(NC) for j in range(i + 1, NC + 1)][:NB]

    def baseline():
        state["pairs"] = [pair(i, j) for i, j in pairs]

    gametes(), table(), parentage(), baseline()
    z = state["z"].cpu().numpy()
    res = {"ploidy": K, "records": NR, "candidates": NC, "progeny": NP, "units": U, "genotypes": G, "gametes": NA, "reads": R, "haplotypes": H,
           "inbreeding": F, "gamete_error": E, "reps": reps, "launches_per_window": per, "baseline_pairs": len(pairs),
           "workspace_bytes": par.workspace_bytes(NR, NP, NC + 1, NC + 1, H, t, t)}
    tab0 = state["table"][0].cpu().numpy()
    host = llk_c[:2 * G].cpu().numpy().reshape(2, G)
    want = np.stack([application.parentage_unit(tab0, tab0, host[c], H, t, t) for c in range(2)])
    res["max_deviation_from_host_definition"] = float(np.max(np.abs(z[0, :2] - want)))
    res["max_deviation_of_the_timed_pairs_from_the_parentage_launch"] = float(max(
        np.max(np.abs(got.cpu().numpy().reshape(NR, NP) - z[:, :, i, j])) for (i, j), got in zip(pairs, state["pairs"])))
    windows = {}
    for name, fn, k in (("likelihood_pass_ms", batch.run_llks64, 1), ("gamete_launch_ms", gametes, per), ("table_ms", table, per),
                        ("parentage_launch_ms", parentage, per), ("baseline_pairs_ms", baseline, 1)):
        windows[name] = timed(fn, k)
    # ... and the launch once more: the spread between the two windows is the noise of the session
    res["parentage_launch_ms_second_window"] = timed(parentage, per)[0]
    for name, (med, lo, hi) in windows.items():
        res[name] = med
        res[name + "_range"] = [lo, hi]
    res["baseline_ms_per_pair"] = res["baseline_pairs_ms"] / len(pairs)
    res["baseline_ms_scaled_to_136_hypotheses"] = res["baseline_ms_per_pair"] * 136
    res["baseline_over_parentage_launch"] = res["baseline_ms_scaled_to_136_hypotheses"] / res["parentage_launch_ms"]
    return res


for K in ploidies:
    print(json.dumps(once(K)), flush=True)
