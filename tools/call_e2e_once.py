"""Measurement aid: `mchap call` and `mchap call-exact` end to end on a synthetic job -- assemble writes the haplotype VCF of `loci`
targets x `samples` samples, the programs re-call every sample against it (files -> VCF records) --
  * `call` through the command line with the traces summarised on the device (CallingMCMC.fit_batch_summaries, round 5) and, for
    comparison, by the host classes on downloaded traces as before;
  * `call` and `call-exact` through mchap_amd.application with block_path=False (reads fetched and encoded record by record, the
    float tensors filled on the host) and with block_path=True (the block path: mchap_amd/blockpath.py, int8 calls uploaded, the read
    tensors formed on the device), `reps` times each: the median rate of both and whether the record lines are equal.
Usage: python tools/call_e2e_once.py [loci] [samples] [reps] [call|call-exact|both] [profile] [phred]
(`profile`: a cProfile of one more run of each program on the block path, by cumulative time; `phred`: the two legs with base
qualities in use -- per record against block_path="wide", int16 qualities uploaded with the calls -- and nothing else)"""
import io as _io, os, sys, time, tempfile, shutil, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mchap_amd import application, cli, synth
from mchap_amd.calling_mcmc import CallingMCMC, CallSummary

n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 4
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
which = sys.argv[4] if len(sys.argv) > 4 else "both"
profile = "profile" in sys.argv[5:]
phred = "phred" in sys.argv[5:]
HAS_BLOCK_PATH = "block_path" in application.call.__code__.co_varnames   # (the same script measures a commit without it)
d = tempfile.mkdtemp(prefix="mchap_call_e2e_")
try:
    job = synth.synth_assembly_inputs(d, n_loci=n, n_samples=ns, reads_per_locus=60)
    vcf = os.path.join(d, "haplotypes.vcf")
    out = _io.StringIO()
    cli.run(["mchap_amd", "assemble", "--bam"] + job["bams"] + ["--targets", job["bed"], "--variants", job["vcf"], "--reference", job["fasta"], "--ploidy", "4"], out)
    open(vcf, "w").write(out.getvalue())
    if which in ("both", "call") and not phred:
        argv = ["mchap_amd", "call", "--bam"] + job["bams"] + ["--haplotypes", vcf, "--ploidy", "4"]
        device = CallingMCMC.start_batch_summaries

        def by_host(self, reads, read_counts=None, initial=None, haplotypes=None, prior=None, stream_ids=None, burn=0, incongruence_threshold=0.6, max_states=512,
                    stream=None):
            return dict(done=[CallSummary.of_trace(t.burn(burn), incongruence_threshold) for t in self.fit_batch(reads, read_counts, initial, haplotypes, prior, stream_ids)])

        texts = {}
        for name, fn in (("device summaries", device), ("host classes", by_host), ("device summaries", device)):
            CallingMCMC.start_batch_summaries = fn
            o = _io.StringIO()
            t0 = time.perf_counter()
            cli.run(argv, o)
            dt = time.perf_counter() - t0
            recs = [l for l in o.getvalue().splitlines() if not l.startswith("#")]
            texts[name] = recs
            print("%-17s %d records x %d samples  %.1f ms  %.0f units/s" % (name, len(recs), ns, dt * 1e3, len(recs) * ns / dt), flush=True)
        CallingMCMC.start_batch_summaries = device
        print("same records:", texts["device summaries"] == texts["host classes"])

    # ---- the block path against the per-record path, both programs ----
    source = application.ReadSource({os.path.basename(b)[:-4]: b for b in job["bams"]}, use_phred=phred)
    for bam in source.bams.values():
        bam.columns()   # (the files inflated and parsed once, outside the timed legs: both paths share the columns)
    programs = [p for p in (("call", application.call), ("call-exact", application.call_exact)) if which in ("both", p[0])]
    for name, fn in programs:
        legs = (("per record", dict(block_path=False)), ("block path", dict(block_path="wide" if phred else True))) if HAS_BLOCK_PATH else (("per record", dict()),)
        lines, rate = {}, {}
        for leg, kw in legs:
            list(fn(vcf, source, ploidy=4, **kw))   # (warm-up: streams, allocator, first launches)
            dts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                lines[leg] = list(fn(vcf, source, ploidy=4, **kw))
                dts.append(time.perf_counter() - t0)
            rate[leg] = len(lines[leg]) * ns / statistics.median(dts)
            print("%-10s %-10s %d records x %d samples  median of %d: %.1f ms  %.0f units/s  (runs: %s)" % (
                name, leg, len(lines[leg]), ns, reps, statistics.median(dts) * 1e3, rate[leg], " ".join("%.1f" % (x * 1e3) for x in dts)), flush=True)
        if HAS_BLOCK_PATH:
            print("%-10s block path / per record: %.2fx   same records: %s" % (name, rate["block path"] / rate["per record"],
                                                                              lines["block path"] == lines["per record"]), flush=True)
        if profile:
            import cProfile, pstats

            pr = cProfile.Profile()
            pr.enable()
            list(fn(vcf, source, ploidy=4, **legs[-1][1]))
            pr.disable()
            pstats.Stats(pr, stream=sys.stdout).sort_stats("cumulative").print_stats(28)
finally:
    shutil.rmtree(d, ignore_errors=True)
