"""The identity evidence of call-exact (--identity) on one GPU: 16 haplotypes, 500 reads, 256 samples a record -- tetraploid over
32 records, hexaploid over 8.  Timed: ms of the one likelihood pass (llks64 alone), ms of the evidence launch for log Z, ms of the
launches that form log pi / 2 and the rows a, ms of the product and combine launches over them -- all 256 x 256 / 2 pairs of every
record --, and for comparison ms of the way to the same numbers without them: llks64 read back over PCIe (that leg is in the
figure, and stated on its own), then application.identity_unit in numpy, timed over the first `baseline records` records and
scaled to all.  The product's float64 rate counts n (n + 1) / 2 x G multiply-adds a record -- the pairs on or above the diagonal,
not the padding of the tiles -- as 2 flops each, against the part's vector FP64 peak of 78.6 TFLOP/s.  The values are checked
against the host definition on the timed records.  HIP events, every figure the median of `reps` windows after a warm-up.  One
JSON line per ploidy.
python tools/identity_once.py [reps] [launches per window] [baseline records] [ploidy:records ...]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import application
from mchap_amd.device import ExactDeviceBatch, ExactIdentity, ExactModelEvidence
from mchap_amd.synth import synth_units

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
per = int(sys.argv[2]) if len(sys.argv) > 2 else 3
NBASE = int(sys.argv[3]) if len(sys.argv) > 3 else 2
runs = [tuple(int(x) for x in a.split(":")) for a in sys.argv[4:]] or [(4, 32), (6, 8)]
NS = 256                 # samples a record
H, M, R = 16, 8, 500
F, E = 0.1, 0.01
PEAK_FP64_VECTOR = 78.6e12


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


def once(K, NR):
    U = NR * NS
    rng = np.random.default_rng(4)
    reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, window=(5, 10), first_unit=400)
    haps = np.unique(rng.integers(0, 2, size=(64, M)).astype(np.int8), axis=0)[:H]
    haps[0] = 0   # (haplotype 0 is REF: allele 0 at every SNV)
    f = rng.dirichlet(np.full(H, 2.0), size=NR)
    batch = ExactDeviceBatch(reads, K, haps, None, None, cache_joint=False)
    llks = batch.run_llks64()   # the units record by record: [NR][NS][G]
    torch.cuda.synchronize()
    G = batch.G
    ident, ev = ExactIdentity(), ExactModelEvidence()
    d_f = torch.from_numpy(f).to(ident.device)
    unit_rows = np.repeat(np.arange(NR, dtype=np.int32), NS)
    rows = np.arange(NR)
    grid = np.full((U, 1), F)
    wsb = ident.workspace_bytes(NR, NS, H, K)
    ws = torch.empty(wsb, dtype=torch.uint8, device=ident.device)
    state = {}

    def evidence():
        state["norm"] = ev.add_group(llks, H, K, grid, unit_rows, d_f).view(NR, NS)

    def form_a():
        ident.log_bayes_factors(llks, H, K, F, rows, d_f, state["norm"], E, phases=1, workspace=ws)

    def product():
        state["lbf"] = ident.log_bayes_factors(llks, H, K, F, rows, d_f, state["norm"], E, phases=2, workspace=ws)

    def readback():
        state["host"] = llks[:NBASE * NS * G].cpu().numpy().reshape(NBASE, NS, G)

    def baseline():
        readback()
        state["want"] = np.stack([application.identity_unit(
            state["host"][r], application._host_log_prior(application._genotype_table(H, K), H, K, F, f[r]), E) for r in range(NBASE)])

    evidence(), form_a(), product()
    got = state["lbf"].cpu().numpy()
    whole = ident.log_bayes_factors(llks, H, K, F, rows, d_f, state["norm"], E).cpu().numpy()
    res = {"ploidy": K, "records": NR, "samples": NS, "units": U, "genotypes": G, "reads": R, "haplotypes": H, "inbreeding": F, "error": E,
           "reps": reps, "launches_per_window": per, "baseline_records": NBASE, "workspace_bytes": wsb,
           "phases_equal_the_whole_call": bool(np.array_equal(got.view(np.uint64), whole.view(np.uint64)))}
    windows = {}
    for name, fn, k in (("likelihood_pass_ms", batch.run_llks64, 1), ("evidence_launch_ms", evidence, per), ("rows_a_launch_ms", form_a, per),
                        ("product_launch_ms", product, per), ("readback_ms", readback, 1)):
        windows[name] = timed(fn, k)
    res["product_launch_ms_second_window"] = timed(product, per)[0]   # (the spread between the two windows: the noise of the session)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        baseline()
        host.append((time.perf_counter() - t0) * 1e3)
    windows["baseline_ms"] = (float(np.median(host)), float(min(host)), float(max(host)))
    off = ~np.eye(NS, dtype=bool)
    res["max_deviation_from_host_definition"] = float(np.max(np.abs(got[:NBASE][:, off] - state["want"][:, off])))
    for name, (med, lo, hi) in windows.items():
        res[name] = med
        res[name + "_range"] = [lo, hi]
    res["readback_ms_scaled_to_all_records"] = res["readback_ms"] / NBASE * NR
    res["baseline_ms_scaled_to_all_records"] = res["baseline_ms"] / NBASE * NR
    res["identity_launches_ms"] = res["rows_a_launch_ms"] + res["product_launch_ms"]
    res["baseline_over_identity_launches"] = res["baseline_ms_scaled_to_all_records"] / res["identity_launches_ms"]
    flops = 2.0 * NR * (NS * (NS + 1) // 2) * G
    res["product_tflops"] = flops / (res["product_launch_ms"] * 1e-3) / 1e12
    res["product_share_of_fp64_vector_peak"] = flops / (res["product_launch_ms"] * 1e-3) / PEAK_FP64_VECTOR
    return res


for K, NR in runs:
    print(json.dumps(once(K, NR)), flush=True)
