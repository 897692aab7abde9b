"""The block path of `mchap call` / `mchap call-exact` on the host side (mchap_amd/blockpath.py, application._exact_units) against
the per-record functions it replaces: the same calls, depths, distinct call rows and counts for every (record, sample); the
compact arrays of a shape group, expanded by the rule of mchap_call_reads_from_calls_device, equal to the tensor the programs'
fill loop builds; and which sources take the path.  No GPU here: tests/test_gpu_call_blockpath.py has the kernel and the
programs' lines."""
import os

import numpy as np
import pytest

from mchap_amd import application, blockpath, encoding, io, synth
from tests.call_blockpath_jobs import HERE, REFERENCE_JOBS, SAMPLES, haplotype_vcf, reference_bams


def _units_both_ways(vcf, source, prior_tag=None):
    _, records = io.read_vcf(vcf)
    slow = application._exact_units(records, source, source.samples, prior_tag, None, False)
    fast = application._exact_units(records, source, source.samples, prior_tag, None, True)
    assert len(slow) == len(fast) == len(records)
    return slow, fast


def _same_inputs(slow, fast, samples):
    """Cell for cell: calls, per-SNV depth, distinct call rows in order of first appearance, their counts (and, where a record
    has variable positions, the float rows formed from them on demand)."""
    n = 0
    for a, b in zip(slow, fast):
        assert a["invalid"] == b["invalid"] and a["needs_kernel"] == b["needs_kernel"]
        M = len(a["locus"].positions)
        for s in samples:
            x, y = a["reads"][s], b["reads"][s]
            assert x["calls"].shape == y["calls"].shape and x["calls"].dtype == y["calls"].dtype
            np.testing.assert_array_equal(x["calls"], y["calls"])
            np.testing.assert_array_equal(np.asarray(x["depth"], dtype=np.int64), np.asarray(y["depth"], dtype=np.int64))
            assert len(x["depth"]) == len(y["depth"]) == M
            np.testing.assert_array_equal(x["counts"], y["counts"])
            if M:
                ucalls, counts = encoding.unique_counts(np.ascontiguousarray(x["calls"]))
                if len(x["calls"]):
                    np.testing.assert_array_equal(ucalls, y["ucalls"])
                    np.testing.assert_array_equal(counts, y["counts"])
                else:
                    assert y["ucalls"].shape == (0, M) and len(y["counts"]) == 0
                assert x["dists"].shape == y["dists"].shape
                assert np.array_equal(x["dists"], y["dists"], equal_nan=True)
            n += len(x["calls"])
    return n


@pytest.mark.parametrize("vcf,bams", REFERENCE_JOBS)
def test_reference_records_encode_the_same(vcf, bams):
    source = application.ReadSource(reference_bams(bams))
    slow, fast = _units_both_ways(os.path.join(HERE, vcf), source)
    assert all(u["block"] is not None for u in fast) and all(u["block"] is None for u in slow)
    assert _same_inputs(slow, fast, SAMPLES) > 50


@pytest.fixture(scope="module")
def synth_job(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("call_block"))
    job = synth.synth_assembly_inputs(d, n_loci=20, n_samples=3, reads_per_locus=14, n_snvs=5, gap=30)
    job["haps"] = haplotype_vcf(job, os.path.join(d, "haps.vcf"), specials=True)
    job["samples"] = ["S000", "S001", "S002"]
    return job


def test_synthetic_job_encodes_the_same(synth_job, tmp_path):
    source = application.ReadSource(dict(zip(synth_job["samples"], synth_job["bams"])))
    slow, fast = _units_both_ways(synth_job["haps"], source, "AFP")
    assert _same_inputs(slow, fast, synth_job["samples"]) > 20 * 3 * 10
    assert [u["invalid"] for u in fast[-3:]] == [None, None, "AF0"] and len(fast[-3]["locus"].positions) == 0
    assert fast[-2]["locus"].mask_reference_allele
    assert max(max(u["locus"].n_alleles, default=0) for u in fast) == 3   # (positions of a record differ in their alleles)
    # overlapping mates: agreeing (one call), disagreeing ('N': no allele), a third record of the name; a deletion; a read of
    # another sample; a record on a contig the file does not have
    recs = [dict(qname="p", flag=0, ref=0, pos=105, mapq=60, cigar=[(30, "M")], seq="A" * 5 + "C" + "A" * 9 + "G" + "A" * 14, qual=[30] * 30, rg="g"),
            dict(qname="q", flag=0, ref=0, pos=106, mapq=60, cigar=[(10, "M"), (3, "D"), (20, "M")], seq="A" * 4 + "C" + "A" * 25, qual=[25] * 30, rg="g"),
            dict(qname="p", flag=0, ref=0, pos=108, mapq=60, cigar=[(2, "S"), (28, "M")], seq="TT" + "A" * 2 + "C" + "A" * 9 + "A" + "A" * 15, qual=[20] * 30, rg="g"),
            dict(qname="p", flag=0, ref=0, pos=109, mapq=60, cigar=[(30, "M")], seq="A" + "C" + "A" * 9 + "T" + "A" * 18, qual=[7] * 30, rg="g"),
            dict(qname="z", flag=0, ref=0, pos=118, mapq=60, cigar=[(30, "M")], seq="AAT" + "A" * 9 + "T" + "A" * 17, qual=[9] * 30, rg="h")]
    bam = str(tmp_path / "pair.bam")
    synth.write_bam(bam, [("chrS", 1000)], {"g": "X", "h": "Y"}, recs)
    ref = "A" * 40
    alts = [ref[:10] + "C" + ref[11:20] + "G" + ref[21:], ref[:10] + "C" + ref[11:20] + "T" + ref[21:30] + "T" + ref[31:]]
    vcf = str(tmp_path / "pair.vcf")
    open(vcf, "w").write("##fileformat=VCFv4.3\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                         "chrS\t101\t.\t%s\t%s\t.\t.\t.\nchrS\t116\t.\t%s\t%s\t.\t.\t.\nnowhere\t5\t.\tAC\tAT\t.\t.\t.\n" % (
                             ref, ",".join(alts), ref[15:], ",".join(a[15:] for a in alts)))
    source = application.ReadSource({"X": bam, "Y": bam})
    slow, fast = _units_both_ways(vcf, source)
    assert _same_inputs(slow, fast, ["X", "Y"]) == 3 + 3 + 0
    assert (fast[0]["reads"]["X"]["calls"] < 0).any() and fast[0]["locus"].n_alleles == [2, 3, 2]


def _fill_loop(units, members, Rmax, M, A):
    """The [U, Rmax, M, A] tensor and [U, Rmax] counts as application._run_exact_groups / call fill them record by record."""
    reads = np.full((len(members), Rmax, M, A), np.nan)
    counts = np.zeros((len(members), Rmax), dtype=np.int64)
    for i, (ri, s) in enumerate(members):
        sr = units[ri]["reads"][s]
        n = len(sr["dists"])
        if n:
            reads[i, :n] = sr["dists"]
            counts[i, :n] = sr["counts"]
    return reads, counts


def test_unit_inputs_expand_to_the_fill_loops_tensor(synth_job):
    source = application.ReadSource(dict(zip(synth_job["samples"], synth_job["bams"])))
    _, records = io.read_vcf(synth_job["haps"])
    # a record nobody has reads for: its units have no rows
    records.append(dict(records[0], chrom="elsewhere"))
    slow = application._exact_units(records, source, source.samples, None, None, False)
    fast = application._exact_units(records, source, source.samples, None, None, True)
    blk = fast[0]["block"]
    groups = {}
    for ri, u in enumerate(fast):
        M = len(u["locus"].positions)
        if M:
            for s in source.samples:
                groups.setdefault((M, max(u["locus"].n_alleles)), []).append((ri, s))
    seen_empty = seen_ragged = False
    for (M, A), members in groups.items():
        members = members[::-1]   # (any order of units, samples interleaved)
        li = np.array([fast[ri]["li"] for ri, _ in members])
        si = np.array([blk["si"][s] for _, s in members])
        calls, counts, rows, c_off, n_off, nal = blockpath.call_unit_inputs(blk["encs"], li, si, blk["nal"])
        assert calls.dtype == np.int8 and counts.dtype == np.int64 and nal.shape == (len(members), M) and nal.dtype == np.int8
        assert len(calls) == int(rows.sum()) * M and len(counts) == int(rows.sum())
        np.testing.assert_array_equal(c_off, np.cumsum(rows * M) - rows * M)
        np.testing.assert_array_equal(n_off, np.cumsum(rows) - rows)
        for i, (ri, _) in enumerate(members):
            assert nal[i].tolist() == fast[ri]["locus"].n_alleles
        for Rmax in (max(int(rows.max()), 1), int(rows.max()) + 3):
            want_reads, want_counts = _fill_loop(slow, members, Rmax, M, A)
            got_reads, got_counts = blockpath.expand_call_units(calls, counts, rows, c_off, n_off, nal, Rmax, A, error_rate=source.error_rate)
            assert got_reads.dtype == np.float64 and got_counts.dtype == np.int64
            assert np.array_equal(got_reads, want_reads, equal_nan=True)
            np.testing.assert_array_equal(got_counts, want_counts)
        seen_empty |= bool((rows == 0).any())
        seen_ragged |= len(set(rows[rows > 0].tolist())) > 1
    assert seen_empty and seen_ragged


def test_expand_rule_small_case():
    """The rule of include/mchap_hip.h spelled out: padding rows, an empty unit, zero after NaN, a call of the last allele."""
    calls = np.array([[1, -1, 0]] + [[0, 2, 1], [-1, -1, -1], [1, 0, -1], [0, 1, 0], [1, 2, 1]], dtype=np.int8)
    counts = np.array([7, 1, 2, 3, 4, 5])
    nal = np.tile(np.array([2, 3, 2], dtype=np.int8), (3, 1))
    reads, rc = blockpath.expand_call_units(calls.reshape(-1), counts, [0, 1, 5], [0, 0, 3], [0, 0, 1], nal, 5, 3, error_rate=0.01)
    p, q = 1.0 - 0.01, (1.0 - (1.0 - 0.01)) / 3.0
    assert np.isnan(reads[0]).all() and rc[0].tolist() == [0] * 5
    assert np.array_equal(reads[1, 0], [[q, p, 0.0], [np.nan, np.nan, np.nan], [p, q, 0.0]], equal_nan=True)
    assert np.isnan(reads[1, 1:]).all() and rc[1].tolist() == [7, 0, 0, 0, 0]
    assert np.array_equal(reads[2, 1], [[np.nan, np.nan, 0.0], [np.nan] * 3, [np.nan, np.nan, 0.0]], equal_nan=True)
    assert np.array_equal(reads[2, 4], [[q, p, 0.0], [q, q, p], [q, p, 0.0]]) and rc[2].tolist() == [1, 2, 3, 4, 5]
    for u, (a, b) in enumerate([(0, 0), (0, 1), (1, 6)]):
        want = encoding.encode_read_distributions([2, 3, 2], calls[a:b], None, error_rate=0.01)
        assert np.array_equal(reads[u, : b - a], want.reshape(b - a, 3, 3), equal_nan=True)


class _Spy:
    """Counts the calls of a source's per-record reads()."""

    def __init__(self, source):
        self.n = 0
        inner = source.reads

        def reads(locus, sample):
            self.n += 1
            return inner(locus, sample)
        source.reads = reads


class _Replay:
    """A `calling=` backend that evaluates nothing: every unit gets the first genotype (what the record lines need)."""

    @staticmethod
    def posterior_mode(dists, ploidy, haps, read_counts=None, prior=None, **kw):
        assert dists.ndim == 3 and len(dists) == len(read_counts)
        H = len(haps)
        return np.zeros(ploidy, int), 0.0, 0.5, 0.75, np.full(H, 1.0 / H), np.full(H, 0.5)


@pytest.mark.parametrize("by_default", [False, True])
def test_which_sources_take_the_block_path(by_default, monkeypatch):
    """by_default: application.CALL_BLOCK_PATH_DEFAULT, what block_path=None means where the source takes the block path."""
    monkeypatch.setattr(application, "CALL_BLOCK_PATH_DEFAULT", by_default)
    vcf = os.path.join(HERE, "simple.output.mixed_depth.assemble.vcf")
    paths = reference_bams(REFERENCE_JOBS[2][1])
    # one file per sample, qualities ignored: no per-record read at all, and the same lines as record by record
    plain = application.ReadSource(paths)
    spy = _Spy(plain)
    fast = list(application.call_exact(vcf, plain, calling=_Replay, block_path=True))
    assert spy.n == 0 and len(fast) > 0
    slow = list(application.call_exact(vcf, plain, calling=_Replay, block_path=False))
    assert spy.n == len(fast) * 3 and slow == fast
    # block_path=None: the block path (no per-record read) where it is the default, else every unit read record by record
    spy.n = 0
    assert list(application.call_exact(vcf, plain, calling=_Replay)) == fast
    assert spy.n == (0 if by_default else len(fast) * 3)
    # several blocks
    spy.n = 0
    assert list(application.call_exact(vcf, plain, calling=_Replay, records_per_block=1, block_path=True)) == fast and spy.n == 0
    # pooled samples, base qualities in use: the per-record path under None, an error when the block path is demanded
    pooled = application.ReadSource({"POOL": [(s, p) for s, p in paths.items()]})
    phred = application.ReadSource(paths, use_phred=True)
    for source, n_samples in ((pooled, 1), (phred, 3)):
        assert not application._block_path_takes(source)
        spy = _Spy(source)
        lines = list(application.call_exact(vcf, source, calling=_Replay))
        assert spy.n == len(lines) * n_samples
        for program in (application.call_exact, application.call):
            with pytest.raises(ValueError, match="block_path=True"):
                list(program(vcf, source, block_path=True))


@pytest.mark.parametrize("block_path", [True, None])
def test_a_block_the_array_path_refuses_goes_record_by_record(block_path, monkeypatch):
    """BlockPathUnavailable inside a block (here: every block) sends that block through the per-record path: under
    block_path=True, and under None where the block path is the default."""
    monkeypatch.setattr(application, "CALL_BLOCK_PATH_DEFAULT", True)
    vcf = os.path.join(HERE, "simple.output.assemble.vcf")
    source = application.ReadSource(reference_bams(REFERENCE_JOBS[0][1]))
    want = list(application.call_exact(vcf, source, calling=_Replay, block_path=False))
    spy = _Spy(source)
    assert list(application.call_exact(vcf, source, calling=_Replay, block_path=block_path)) == want and spy.n == 0
    refused = []

    def refuse(*a, **kw):
        refused.append(1)
        raise blockpath.BlockPathUnavailable("row hash collision")
    monkeypatch.setattr(blockpath, "encode_block", refuse)
    assert list(application.call_exact(vcf, source, calling=_Replay, block_path=block_path, records_per_block=2)) == want
    assert spy.n == len(want) * 3 and len(refused) == (len(want) + 1) // 2   # (asked once per block, every unit then read per record)
    # one block refused, the others taken
    monkeypatch.undo()
    monkeypatch.setattr(application, "CALL_BLOCK_PATH_DEFAULT", True)
    inner, seen = blockpath.encode_block, []

    def refuse_the_second(*a, **kw):
        seen.append(1)
        if len(seen) == 4:   # (three samples: the first sample of the second block, which holds one record)
            raise blockpath.BlockPathUnavailable("row hash collision")
        return inner(*a, **kw)
    monkeypatch.setattr(blockpath, "encode_block", refuse_the_second)
    spy.n = 0
    assert list(application.call_exact(vcf, source, calling=_Replay, block_path=block_path, records_per_block=len(want) - 1)) == want
    assert spy.n == 1 * 3


def test_matrix_source_goes_the_block_path_too(synth_job):
    """A MatrixSource (pileup matrices keyed by (record id, sample)) through both paths: the same inputs, the same lines."""
    bams = application.ReadSource(dict(zip(synth_job["samples"], synth_job["bams"])))
    _, records = io.read_vcf(synth_job["haps"])
    units = application._exact_units(records, bams, bams.samples, None, None, False)
    matrices = {(u["locus"].name, s): (u["reads"][s]["chars"], np.zeros(u["reads"][s]["chars"].shape, dtype=np.int16)) for u in units for s in bams.samples}
    assert len(matrices) == len(records) * 3
    source = application.MatrixSource(bams.samples, matrices)
    assert application._block_path_takes(source)
    slow, fast = _units_both_ways(synth_job["haps"], source, "AFP")
    assert all(u["block"] is not None for u in fast)
    assert _same_inputs(slow, fast, bams.samples) > 20 * 3 * 10
    want = list(application.call_exact(synth_job["haps"], bams, calling=_Replay, block_path=False))
    spy = _Spy(source)
    assert list(application.call_exact(synth_job["haps"], source, calling=_Replay, block_path=True)) == want and spy.n == 0
    assert not application._block_path_takes(application.MatrixSource(bams.samples, matrices, use_phred=True))


def test_call_reports_likelihoods_of_a_record_without_variable_positions(tmp_path):
    """`call --report GL` on a record whose haplotypes do not differ: one genotype, likelihood 1 (log10: 0) whatever the reads
    -- what call-exact writes; the exact caller itself takes no tensor without positions.  Nothing here reaches the device."""
    vcf = str(tmp_path / "flat.vcf")
    open(vcf, "w").write("##fileformat=VCFv4.3\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nCHR1\t8\t.\tACGTACGT\t.\t.\t.\t.\n")
    source = application.ReadSource(reference_bams(REFERENCE_JOBS[0][1]))
    # (call-exact's line with the MCI column as call writes it: a sampler statistic there, "." here)
    want = [ln.replace(":1:1:.:0", ":1:1:0:0") for ln in application.call_exact(vcf, source, ploidy=2, report=("GL",), block_path=False)]
    for block_path in (False, True):
        got = list(application.call(vcf, source, ploidy=2, report=("GL",), steps=20, burn=10, block_path=block_path))
        assert got == want and got[0].split("\t")[8].endswith(":GL") and got[0].split("\t")[9].endswith(":0")
