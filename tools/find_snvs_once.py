"""find-snvs on a synthetic population: kernel time per block (HIP events), the host split (inflate / segment tables / record
formatting) and records/s end to end, the LDS-histogram depth launch against the global-atomic variant on the same blocks, and
the tests' per-read counter (tests/pileup_reference.py) on the same input as a CPU baseline.  Prints one JSON line.

    python tools/find_snvs_once.py [--samples 96] [--targets 400] [--reads 40] [--deep-reads 0] [--dir DIR]

--deep-reads N: amplicon-like depth, N reads per (target, sample) (heavy same-address contention in the histogram)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=96)
    ap.add_argument("--targets", type=int, default=400)
    ap.add_argument("--reads", type=int, default=40, help="reads per (target, sample)")
    ap.add_argument("--deep-reads", type=int, default=0)
    ap.add_argument("--cpu-samples", type=int, default=2, help="samples the per-read CPU counter is timed on")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from mchap_amd import application, find_snvs, io, synth

    reads = a.deep_reads or a.reads
    d = a.dir or tempfile.mkdtemp(prefix="find_snvs_")
    t0 = time.perf_counter()
    job = synth.synth_assembly_inputs(d, n_loci=a.targets, n_samples=a.samples, reads_per_locus=reads)
    t_synth = time.perf_counter() - t0
    samples = ["S%03d" % i for i in range(a.samples)]
    source = application.ReadSource(dict(zip(samples, job["bams"])), workers=8)
    reference = io.Reference(job["fasta"])
    targets = find_snvs.read_targets(job["bed"])
    torch.cuda.init()
    out = dict(samples=a.samples, targets=len(targets), reads_per_target_sample=reads, positions=int(sum(b - s for _, s, b in targets)))
    # warm-up (library load, first launches), then the timed run
    list(find_snvs.find_snvs(targets[:2], reference, source))
    timings = {}
    t0 = time.perf_counter()
    n = sum(1 for _ in find_snvs.find_snvs(targets, reference, source, timings=timings))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    k = find_snvs.kernel_ms(timings)
    out.update(records=n, wall_s=round(wall, 3), records_per_s=round(n / wall, 1), kernel_ms=round(sum(k.values()), 3),
               depth_ms=round(k.get("depth", 0.0), 3), filter_ms=round(k.get("filter", 0.0), 3),
               blocks=len(find_snvs.plan_blocks(targets, find_snvs.block_rows_budget(a.samples))),
               inflate_s=round(timings.get("inflate", 0.0), 3), tables_s=round(timings.get("tables", 0.0), 3),
               format_s=round(timings.get("format", 0.0), 3))
    # the depth launch alone, LDS histogram vs global atomics, on one block of all targets
    files = find_snvs._Files(source)
    windows = [("chrS", s, b) for _, s, b in targets]
    for variant in (0, 1):
        best = None
        for _ in range(3):
            tm = {}
            find_snvs._block_depths(files, windows, variant=variant, timings=tm)
            ms = find_snvs.kernel_ms(tm)["depth"]
            best = ms if best is None else min(best, ms)
        out["depth_ms_variant%d" % variant] = round(best, 3)
    # CPU baseline: the tests' per-read counter on the same input
    import pileup_reference as pr

    t0 = time.perf_counter()
    for s in range(min(a.cpu_samples, a.samples)):
        _, _, recs = io.read_bam(job["bams"][s])
        recs = [dict(r, ref=0, cigar=r["cigar"]) for r in recs]
        for _, st, sp in targets:
            pr.count(recs, 0, st, sp)
    cpu = time.perf_counter() - t0
    out.update(cpu_counter_s_per_sample=round(cpu / max(1, min(a.cpu_samples, a.samples)), 3), synth_s=round(t_synth, 1),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
