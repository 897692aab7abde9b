"""GPU: find-snvs end to end (python -m mchap_amd find-snvs) against the reference's golden VCFs, the device allele depths
against a plain per-read counter, the filter launch against a numpy restatement of the reference's write_vcf_block bit for
bit, and find-snvs -> assemble --variants."""
import io as _io
import os

import numpy as np
import pytest

import pileup_reference as pr

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
SHALLOW = ["simple.sample1.bam", "simple.sample2.bam", "simple.sample3.bam"]
MIXED = ["simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam"]
DEEP = ["simple.sample1.deep.bam", "simple.sample2.deep.bam", "simple.sample3.deep.bam"]
EXEMPT = ("##fileDate", "##source", "##commandline", "##reference")


def _program(bams, extra, bed=None):
    from mchap_amd import cli

    out = _io.StringIO()
    cli.run(["mchap_amd", "find-snvs", "--targets", bed or os.path.join(HERE, "simple.bed"), "--reference",
             os.path.join(HERE, "simple.fasta"), "--bam"] + [os.path.join(HERE, b) for b in bams] + list(extra), out)
    return out.getvalue().splitlines()


@pytest.mark.parametrize("bams,extra,golden", [
    (SHALLOW, [], "simple.output.basis.vcf"),
    (MIXED, [], "simple.output.basis.mixed_depth.vcf"),
    (MIXED, ["--ind-maf", "0", "--ind-mad", "0", "--maf", "0.1"], "simple.output.basis.mixed_depth.maf0.1.vcf"),
    (MIXED, ["--ind-maf", "0", "--ind-mad", "0", "--mad", "10"], "simple.output.basis.mixed_depth.mad10.vcf"),
    (SHALLOW, ["--ind-maf", "0.3"], "simple.output.basis.minaf0.3.vcf"),
    (SHALLOW, ["--ind-mad", "2"], "simple.output.basis.minad2.vcf"),
    (SHALLOW, ["--ind-maf", "0.0", "--ind-mad", "0"], "simple.output.basis.minaf0.minad0.vcf"),
])
def test_program_reproduces_the_reference_goldens(bams, extra, golden):
    got = _program(bams, extra)
    want = [ln.rstrip("\n") for ln in open(os.path.join(HERE, golden))]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w.startswith(EXEMPT):
            assert g.split("=", 1)[0] == w.split("=", 1)[0]
        else:
            assert g == w


def _crafted_source(tmp_path, n_samples=2, read_filter=None):
    from mchap_amd import application, synth

    paths = {}
    recs_of = {}
    for s in range(n_samples):
        contigs, recs = pr.crafted_records(seed=11 + s)
        p = str(tmp_path / ("s%d.bam" % s))
        synth.write_bam(p, contigs, {"rg%d" % s: "S%d" % s}, [dict(r, rg="rg%d" % s) for r in recs])
        paths["S%d" % s] = p
        recs_of["S%d" % s] = recs
    kw = dict(read_filter or {})
    if "min_quality" in kw:
        kw["mapping_quality"] = kw.pop("min_quality")
    source = application.ReadSource(paths, read_group_field="SM", **kw)
    return contigs, source, recs_of


@pytest.mark.parametrize("read_filter", [None, dict(min_quality=0, skip_duplicates=False, skip_qcfail=False, skip_supplementary=False)])
def test_allele_depths_equal_the_per_read_counter(tmp_path, read_filter):
    from mchap_amd import find_snvs

    _, source, recs_of = _crafted_source(tmp_path, 2, read_filter)
    total = 0
    for contig, tid, a, b in (("c1", 0, 0, 700), ("c1", 0, 123, 517), ("c2", 1, 0, 300)):
        want = np.stack([pr.count(recs_of[s], tid, a, b, read_filter) for s in ("S0", "S1")], axis=1)
        total += int(want.sum())
        for tile, variant in ((find_snvs.TILE, 0), (64, 0), (7, 0), (64, 1)):  # tiles smaller than a read: reads cross tile edges
            got = find_snvs.allele_depths(source, contig, a, b, tile=tile, variant=variant)
            assert got.shape == (b - a, 2, 4)
            np.testing.assert_array_equal(got, want, err_msg="%s:%d-%d tile %d variant %d" % (contig, a, b, tile, variant))
    assert total > 1000


def _random_depths(rng, P, S):
    d = rng.integers(0, 6, size=(P, S, 4)) * (rng.random((P, S, 4)) < 0.6)
    d[rng.random((P, S)) < 0.15] = 0              # samples without depth (NaN frequencies)
    d[: P // 8] = d[: P // 8] // 3                # shallow rows: ties
    d[P // 8: P // 4, :, 2:] = d[P // 8: P // 4, :, :2]   # equal alleles: ties in ADMF
    return d.astype(np.int32)


@pytest.mark.parametrize("S", [1, 3, 40, 1000])
@pytest.mark.parametrize("params", [dict(), dict(maf=0.1), dict(maf=0.2, ind_maf=0.0, ind_mad=0), dict(mad=10, ind_maf=0.0, ind_mad=0),
                                    dict(min_ind=2), dict(min_ind=3, ind_maf=0.05, ind_mad=1), dict(ind_maf=0.3), dict(min_ind=0)])
def test_filter_launch_equals_the_numpy_restatement_bit_for_bit(S, params):
    import torch

    from mchap_amd import find_snvs

    rng = np.random.default_rng(S * 1000 + len(params))
    P = 600 if S < 1000 else 150
    d = _random_depths(rng, P, S)
    ref = rng.integers(0, 4, size=P).astype(np.int8)
    ref[rng.random(P) < 0.1] = -1                 # reference bases that are not ACGT
    flags, admf = find_snvs.filter_device(torch.from_numpy(d).cuda(), torch.from_numpy(ref), **params)
    flags, admf = flags.cpu().numpy(), admf.cpu().numpy()
    rows, order, keep, refmasked, f = pr.write_vcf_block_filter(d, ref, **params)
    rec, keep_d, order_d, refmasked_d = find_snvs.decode_flags(flags)
    np.testing.assert_array_equal(np.flatnonzero(rec), rows)
    np.testing.assert_array_equal(order_d[rows], order)
    k = np.take_along_axis(keep_d[rows], order, axis=1)
    k[:, 0] = True
    np.testing.assert_array_equal(k, keep)
    np.testing.assert_array_equal(refmasked_d[rows], refmasked)
    got = np.take_along_axis(admf[rows], order, axis=1)
    assert np.array_equal(np.isnan(got), np.isnan(f))
    assert np.array_equal(np.nan_to_num(got, nan=-1.0).view(np.int64), np.nan_to_num(f, nan=-1.0).view(np.int64))


def test_program_on_synthetic_population_equals_counter_and_filter(tmp_path):
    """Overlapping BED intervals, a zero-coverage target, non-ACGT reference bases, windows and blocks smaller than the intervals,
    tiles smaller than a read: the records equal those of the per-read counter + the numpy filter + the record formatter."""
    from mchap_amd import find_snvs, io

    contigs, source, recs_of = _crafted_source(tmp_path, 3)
    rng = np.random.default_rng(5)
    seqs = {n: "".join(rng.choice(list("ACGT"), size=L)) for n, L in contigs}
    seqs["c1"] = seqs["c1"][:200] + "NNRN" + seqs["c1"][204:]
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(">%s\n%s\n" % kv for kv in seqs.items()))
    reference = io.Reference(str(fa))
    targets = [("c1", 0, 700), ("c1", 150, 260), ("c2", 10, 290), ("c1", 690, 700), ("c1", 180, 210)]
    params = dict(ind_maf=0.05, ind_mad=1)
    got = list(find_snvs.find_snvs(targets, reference, source, **params))
    small = list(find_snvs.find_snvs(targets, reference, source, block_rows=97, tile=16, **params))
    assert got == small
    want = []
    for contig, a, b in targets:
        tid = [n for n, _ in contigs].index(contig)
        d = np.stack([pr.count(recs_of[s], tid, a, b) for s in ("S0", "S1", "S2")], axis=1)
        ref = find_snvs.bases_to_indices(seqs[contig][a:b])
        rows, order, keep, refmasked, f = pr.write_vcf_block_filter(d, ref, **params)
        # (the formatter takes the filter launch's layout: flags and ADMF by allele index)
        inv = np.argsort(order, axis=1)
        k_idx = np.take_along_axis(keep, inv, axis=1)
        k_idx[np.arange(len(rows)), order[:, 0]] = ~refmasked
        flags = 1 | (k_idx.astype(np.int64) << (1 + np.arange(4))).sum(1) | (order << (8 + 2 * np.arange(4))).sum(1) | (refmasked.astype(np.int64) << 16)
        want += find_snvs.format_records([contig] * len(rows), a + rows, d[rows], flags, np.take_along_axis(f, inv, axis=1))
    assert got == want and len(got) > 10
    assert not any(ln.startswith("c1\t20%d\t" % i) for ln in got for i in (1, 2, 3, 4))  # the N / R reference bases


def test_find_snvs_output_feeds_assemble(tmp_path):
    """find-snvs on the deep BAMs, its VCF as assemble --variants: one assembled (non-LIMIT) record per BED target; CHR3 has no
    SNVs and still gets its record, as in the reference's deep assemble golden."""
    from mchap_amd import cli, io

    vcf = tmp_path / "snvs.vcf"
    vcf.write_text("\n".join(_program(DEEP, [])) + "\n")
    samples, recs = io.read_vcf(str(vcf))
    assert samples == ["SAMPLE1", "SAMPLE2", "SAMPLE3"] and len(recs) > 0
    assert {r["chrom"] for r in recs} <= {"CHR1", "CHR2"}
    out = _io.StringIO()
    cli.run(["mchap_amd", "assemble", "--bam"] + [os.path.join(HERE, f) for f in DEEP] + [
        "--ploidy", "4", "--targets", os.path.join(HERE, "simple.bed"), "--variants", str(vcf), "--reference",
        os.path.join(HERE, "simple.fasta"), "--mcmc-steps", "300", "--mcmc-burn", "100", "--mcmc-seed", "11"], out)
    lines = [ln for ln in out.getvalue().splitlines() if ln and not ln.startswith("#")]
    names = [ln.split("\t")[2] for ln in lines]
    assert names == [ln.split()[3] for ln in open(os.path.join(HERE, "simple.bed"))]
    assert all(ln.split("\t")[6] != "LIMIT" for ln in lines)
    chr3 = [ln for ln in lines if ln.startswith("CHR3")]
    assert len(chr3) == 1 and "NVAR=0" in chr3[0]
