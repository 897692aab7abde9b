"""call-exact --model-evidence on the device: the table of a small block against the definition (application.model_evidence_host)
on the library's own float64 likelihoods, per record and host path, after the frequency estimate, the skipping rule, and the record
lines with and without the accumulator."""
import os
from math import comb

import numpy as np
import pytest

from mchap_amd import application
from tests import evidence_reference as ref
from tests.estimate_units import fresh, make_record, per_sample, samples_of

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
SAMPLES = ["SAMPLE1", "SAMPLE2", "SAMPLE3"]
BAMS = ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")
VCF = os.path.join(HERE, "mock.input.frequencies.vcf")
CAND_K, CAND_F = (2, 4), (0.0, 0.1, 0.5)


class Calling64:
    """The `calling` mirror with the library's unrounded likelihoods: genotype_likelihoods in float64 (calling.genotype_likelihoods
    rounds to the reference's float32)."""

    @staticmethod
    def genotype_likelihoods(reads, ploidy, haplotypes, read_counts=None):
        from mchap_amd import _lib, calling

        reads, rc = calling._reads(reads, read_counts)
        haps = np.ascontiguousarray(haplotypes, dtype=np.int8)
        R, M, A = reads.shape
        out32 = np.full(comb(len(haps) + ploidy - 1, ploidy), np.nan, np.float32)
        out64 = np.full(len(out32), np.nan, np.float64)
        _lib.check(_lib.lib().mchap_exact_genotype_likelihoods(_lib.ptr(reads), R, M, A, _lib.ptr(rc), _lib.ptr(haps), len(haps), int(ploidy),
                                                               _lib.ptr(out32), _lib.ptr(out64)))
        return out64


@pytest.fixture(scope="module")
def source():
    """The golden job's pileups as a MatrixSource (keyed by (record id, sample))."""
    bams = application.ReadSource({s: os.path.join(HERE, f) for s, f in zip(SAMPLES, BAMS)})
    _, records = application.read_vcf(VCF)
    units = application._exact_units(records, bams, SAMPLES, "AFP", None, False)
    matrices = {(u["locus"].name, s): (u["reads"][s]["chars"], np.zeros(u["reads"][s]["chars"].shape, dtype=np.int16)) for u in units for s in SAMPLES}
    return application.MatrixSource(SAMPLES, matrices)


def _compare(device, host, cands):
    """The per-unit values of two add_block results: the same units, skipped alike, every value within the kernels' bound."""
    assert sorted(device) == sorted(host)
    worst = 0.0
    for key in host:
        assert (device[key] is None) == (host[key] is None), key
        if host[key] is None:
            continue
        for c, (K, F) in enumerate(cands):
            ok, err = ref.within(device[key][c], host[key][c], F)
            worst = max(worst, err)
            assert ok, (key, K, F, device[key][c], host[key][c])
    return worst


def _in_order_sums(acc, got):
    """The accumulator's sums are its units' values added in record order."""
    for s in acc.samples:
        run, n, skipped = np.zeros(len(acc.candidates[s])), 0, 0
        for ri in sorted({ri for ri, _ in got}):
            if got[(ri, s)] is None:
                skipped += 1
            else:
                run, n = run + got[(ri, s)], n + 1
        assert np.array_equal(run, acc.sums[s]) and acc.records[s] == n and acc.skipped[s] == skipped


@pytest.mark.parametrize("block_path", [False, True])
def test_the_program_against_the_definition(block_path, source):
    kw = dict(ploidy=4, inbreeding=0.1, prior_frequencies_tag="AFP", report=("AFPRIOR", "AFP"), block_path=block_path)
    plain = list(application.call_exact(VCF, source, **kw))
    acc = application.ModelEvidence(SAMPLES, CAND_K, CAND_F, frequency_source="tag AFP")
    assert list(application.call_exact(VCF, source, model_evidence=acc, **kw)) == plain      # the record lines are identical
    assert acc.records_seen == len(plain) and all(acc.records[s] >= 1 and acc.skipped[s] == 0 for s in SAMPLES)
    _, records = application.read_vcf(VCF)
    units = application._exact_units(records, source, SAMPLES, "AFP", None, block_path)
    cands = [(K, F) for K in CAND_K for F in CAND_F]
    dev = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    got = dev.add_block(units, lambda s: 4, lambda s: 0.1)
    host = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    want = host.add_block(units, lambda s: 4, lambda s: 0.1, backend=Calling64)
    worst = _compare(got, want, cands)
    print("block_path %s: %d units, worst |device - definition| %.3g" % (block_path, len(got), worst))
    _in_order_sums(dev, got)
    for s in SAMPLES:
        assert np.array_equal(dev.sums[s], acc.sums[s])                                      # the program's table is this table
        assert [r["configured"] for r in acc.table() if r["sample"] == s] == [0, 0, 0, 0, 1, 0]
    # one record per block: the same sums (record order), bit for bit
    each = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    assert list(application.call_exact(VCF, source, model_evidence=each, records_per_block=1, **kw)) == plain
    assert all(np.array_equal(each.sums[s], acc.sums[s]) for s in SAMPLES)
    # the flat genotype prior
    flat_kw = dict(ploidy=4, block_path=block_path)
    flat = application.ModelEvidence(SAMPLES, CAND_K)
    assert list(application.call_exact(VCF, source, model_evidence=flat, **flat_kw)) == list(application.call_exact(VCF, source, **flat_kw))
    units = application._exact_units(records, source, SAMPLES, None, None, block_path)
    host = application.ModelEvidence(SAMPLES, CAND_K)
    want = host.add_block(units, lambda s: 4, lambda s: None, backend=Calling64)
    got = application.ModelEvidence(SAMPLES, CAND_K).add_block(units, lambda s: 4, lambda s: None)
    _compare(got, want, [(2, None), (4, None)])
    for s in SAMPLES:
        for c in range(2):
            assert ref.within(flat.sums[s][c], host.sums[s][c], None)[0]


def test_pooled_samples_and_the_wide_block_path():
    """--sample-pool and block_path="wide" (base qualities in use): the same table as record by record, the same lines."""
    pools = {"POOL": [(SAMPLES[0], os.path.join(HERE, BAMS[0])), (SAMPLES[2], os.path.join(HERE, BAMS[2]))],
             SAMPLES[1]: [(SAMPLES[1], os.path.join(HERE, BAMS[1]))]}
    names = list(pools)
    cands = [(K, F) for K in CAND_K for F in CAND_F]
    tables = {}
    for block_path in (False, "wide"):
        src = application.ReadSource(pools, use_phred=True)
        kw = dict(ploidy=4, inbreeding=0.1, prior_frequencies_tag="AFP", block_path=block_path, use_base_phred_scores=True)
        acc = application.ModelEvidence(names, CAND_K, CAND_F)
        assert list(application.call_exact(VCF, src, model_evidence=acc, **kw)) == list(application.call_exact(VCF, src, **kw))
        assert all(acc.records[s] == 2 and acc.skipped[s] == 0 for s in names)
        tables[block_path] = acc
    for s in names:
        for c, (K, F) in enumerate(cands):
            assert ref.within(tables["wide"].sums[s][c], tables[False].sums[s][c], F)[0], (s, K, F)
    # ... and with --filter-input-haplotypes: the alleles that are left are the ones the evidence is over
    src = application.ReadSource({s: os.path.join(HERE, f) for s, f in zip(SAMPLES, BAMS)})
    kw = dict(ploidy=4, inbreeding=0.1, prior_frequencies_tag="AFP", filter_input_haplotypes="AFP>=0.1")
    acc = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    assert list(application.call_exact(VCF, src, model_evidence=acc, **kw)) == list(application.call_exact(VCF, src, **kw))
    _, records = application.read_vcf(VCF)
    units = application._exact_units(records, src, SAMPLES, "AFP", application._allele_filter(VCF, "AFP>=0.1"), False)
    assert any(len(u["locus"].haplotypes) < n for u, n in zip(units, (3, 1, 4)))                 # the filter removed an allele
    host = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    host.add_block(units, lambda s: 4, lambda s: 0.1, backend=Calling64)
    for s in SAMPLES:
        assert acc.records[s] == host.records[s] >= 1
        for c, (K, F) in enumerate(cands):
            assert ref.within(acc.sums[s][c], host.sums[s][c], F)[0], (s, K, F)


def test_the_evidence_follows_the_frequency_estimate(source):
    kw = dict(ploidy=4, inbreeding=0.1, prior_frequencies_tag="AFP", report=("AFPRIOR", "AFP"), estimate_frequencies=5)
    acc = application.ModelEvidence(SAMPLES, CAND_K, CAND_F, frequency_source="estimated")
    assert list(application.call_exact(VCF, source, model_evidence=acc, **kw)) == list(application.call_exact(VCF, source, **kw))
    _, records = application.read_vcf(VCF)
    units = application._exact_units(records, source, SAMPLES, "AFP", None, False)
    before = [np.array(u["locus"].frequencies) for u in units]
    est = application.estimate_prior_frequencies(units, SAMPLES, lambda s: 4, lambda s: 0.1, 5)
    assert est and any(not np.array_equal(units[ri]["locus"].frequencies, before[ri]) for ri in est)
    cands = [(K, F) for K in CAND_K for F in CAND_F]
    host = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    want = host.add_block(units, lambda s: 4, lambda s: 0.1, backend=Calling64)
    dev = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    _compare(dev.add_block(units, lambda s: 4, lambda s: 0.1), want, cands)
    plain = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    list(application.call_exact(VCF, source, model_evidence=plain, **dict(kw, estimate_frequencies=None)))
    for s in SAMPLES:
        assert np.array_equal(dev.sums[s], acc.sums[s])            # conditioned on the frequencies the records are called with
        assert not np.array_equal(plain.sums[s], acc.sums[s])


def test_a_unit_beyond_the_budget_or_the_library_is_skipped_for_all(source, monkeypatch):
    kw = dict(ploidy=4, inbreeding=0.1, prior_frequencies_tag="AFP")
    plain = list(application.call_exact(VCF, source, **kw))
    _, records = application.read_vcf(VCF)
    units = application._exact_units(records, source, SAMPLES, "AFP", None, False)
    Hs = {ri: len(u["locus"].haplotypes) for ri, u in enumerate(units) if u["needs_kernel"]}
    big = max(Hs.values())
    assert min(Hs.values()) < big
    cost = application._exact_unit_bytes(comb(big + 4 - 1, 4), 8)
    real = application.device_unit_budget
    # a budget one byte short of the largest record's likelihoods at ploidy 4: that record is skipped -- at ploidy 2 as well
    monkeypatch.setattr(application, "device_unit_budget", lambda b, **k: (cost - 1) // b if b == 1 else real(b, **k))
    acc = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    assert list(application.call_exact(VCF, source, model_evidence=acc, **kw)) == plain      # never FILTER=LIMIT: the lines stay
    monkeypatch.undo()
    n_big = sum(1 for H in Hs.values() if H == big)
    full = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    got = full.add_block(units, lambda s: 4, lambda s: 0.1)
    for s in SAMPLES:
        assert acc.skipped[s] == n_big and acc.records[s] == len(Hs) - n_big
        run = np.zeros(6)
        for ri in sorted(Hs):
            if Hs[ri] != big:
                run = run + got[(ri, s)]
        assert np.array_equal(run, acc.sums[s])
    assert all(r["skipped"] == n_big for r in acc.table())
    # a chunk the library refuses because of ONE of its units: the others are evaluated on their own, only that unit is skipped
    from mchap_amd import device

    target = (sorted(Hs)[0], SAMPLES[1])
    real_add = device.ExactModelEvidence.add_group

    def refusing(self, llks64, n_haps, ploidy, grid, *a):
        res = real_add(self, llks64, n_haps, ploidy, grid, *a)
        cols = [c for c, (K, _) in enumerate([(K, F) for K in CAND_K for F in CAND_F]) if K == ploidy]
        if any(np.array_equal(row, got[target][cols]) for row in res.cpu().numpy()):
            raise NotImplementedError("refused for the test")
        return res

    monkeypatch.setattr(device.ExactModelEvidence, "add_group", refusing)
    one = application.ModelEvidence(SAMPLES, CAND_K, CAND_F)
    part = one.add_block(units, lambda s: 4, lambda s: 0.1)
    monkeypatch.undo()
    assert part[target] is None and all((part[k] is None) == (k == target) for k in got)
    assert all(np.array_equal(part[k], got[k]) for k in got if k != target)
    assert [one.skipped[s] for s in SAMPLES] == [0, 1, 0]
    # a candidate the library does not enumerate (2^62 genotypes or more), on a synthetic block through the device path
    rng = np.random.default_rng(31)
    block = [make_record(rng, 4, 3, (2, 4), (9, 12), name="a"), make_record(rng, 200, 8, (2, 4), (3, 2), name="big"),
             make_record(rng, 5, 3, (2, 4), (0, 7), name="b")]
    dev = application.ModelEvidence(samples_of(block), (2, 15), (0.3,))
    got = dev.add_block(fresh(block), per_sample((2, 4)), per_sample((0.1, 0.3)))
    host = application.ModelEvidence(samples_of(block), (2, 15), (0.3,))
    want = host.add_block(fresh(block), per_sample((2, 4)), per_sample((0.1, 0.3)), backend=Calling64)
    assert all(got[(1, s)] is None for s in samples_of(block)) and np.all(got[(2, "S0")] == 0.0)   # (no reads: exactly 0)
    _compare(got, want, [(2, 0.3), (15, 0.3)])
    assert all(dev.skipped[s] == 1 and dev.records[s] == 2 for s in samples_of(block))
    assert all(u["invalid"] is None for u in block)
