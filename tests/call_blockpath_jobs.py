"""Inputs shared by tests/test_call_blockpath.py and tests/test_gpu_call_blockpath.py (not a test module): the reference's
test files, and haplotype VCFs for `call` / `call-exact` written over a synth.synth_assembly_inputs job without a sampler."""
import os

import numpy as np

from mchap_amd import io

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
SAMPLES = ["SAMPLE1", "SAMPLE2", "SAMPLE3"]
SHALLOW = ["simple.sample1.bam", "simple.sample2.bam", "simple.sample3.bam"]
DEEP = ["simple.sample1.deep.bam", "simple.sample2.deep.bam", "simple.sample3.deep.bam"]
MIXED = ["simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam"]
REFERENCE_JOBS = [("simple.output.assemble.vcf", SHALLOW), ("simple.output.assemble.vcf", DEEP),
                  ("simple.output.mixed_depth.assemble.vcf", MIXED), ("simple.output.mixed_depth.assemble.vcf", DEEP)]


def reference_bams(files):
    return {s: os.path.join(HERE, f) for s, f in zip(SAMPLES, files)}


def haplotype_vcf(job, path, max_alts=3, seed=7, specials=False):
    """A VCF of known haplotypes over the targets of a synth.synth_assembly_inputs job: per target the reference window and up
    to max_alts alternates that differ from it at some of the target's SNVs (mostly by the SNV's alternate base; now and then
    by a third base, so that positions of a record differ in their numbers of alleles), with prior frequencies in INFO/AFP.
    specials: the list then ends with a record without alternates (no variable position), a REFMASKED record and a record
    whose prior frequencies are all zero (AF0 under --prior-frequencies AFP)."""
    rng = np.random.default_rng(seed)
    _, variants = io.read_vcf(job["vcf"])
    ref = io.Reference(job["fasta"])
    by = {}
    for v in variants:
        by.setdefault(v["chrom"], []).append(v)
    lines = ["##fileformat=VCFv4.3", '##INFO=<ID=AFP,Number=R,Type=Float,Description="prior allele frequencies">',
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    targets = io.read_bed4(job["bed"])
    for ti, (contig, start, stop, name) in enumerate(targets):
        seq = ref.fetch(contig, start, stop)
        snvs = [v for v in by.get(contig, []) if start < v["pos"] <= stop]
        alts = []
        for _ in range(int(rng.integers(1, max_alts + 1))):
            chars = list(seq)
            for v in snvs:
                x = rng.random()
                if x < 0.45:
                    chars[v["pos"] - 1 - start] = v["alts"][0]
                elif x < 0.5:
                    chars[v["pos"] - 1 - start] = [c for c in "ACGT" if c not in (v["ref"], v["alts"][0])][0]
            alt = "".join(chars)
            if alt != seq and alt not in alts:
                alts.append(alt)
        if not alts:   # (every draw came out as the reference window: the first SNV's alternate base)
            v = snvs[0]
            alts.append(seq[: v["pos"] - 1 - start] + v["alts"][0] + seq[v["pos"] - start:])
        info = "AFP=" + ",".join("%.3f" % f for f in rng.dirichlet(np.ones(len(alts) + 1)) + 0.001)
        kind = len(targets) - 1 - ti if specials else -1
        if kind == 2:
            alts, info = [], "AFP=1"
        elif kind == 1:
            info = "REFMASKED;" + info
        elif kind == 0:
            info = "AFP=" + ",".join(["0"] * (len(alts) + 1))
        lines.append("\t".join([contig, str(start + 1), name, seq, ",".join(alts) if alts else ".", ".", ".", info]))
    open(path, "w").write("\n".join(lines) + "\n")
    return path
