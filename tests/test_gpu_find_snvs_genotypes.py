"""GPU: find-snvs genotype calls (mchap_snv_genotypes_device) against the numpy definition (snv_genotype_reference.py) on tensors
laid out as the depth and filter launches leave them, and find-snvs end to end with and without calls."""
import io as _io
import os
from functools import lru_cache

import numpy as np
import pytest

import snv_genotype_reference as sg

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
BAMS = [os.path.join(HERE, "simple.sample%d.bam" % i) for i in (1, 2, 3)]
P = 37                  # rows: not a multiple of a wavefront
ZERO_FREQUENCY_ROW = 5  # a record with a kept alternate whose ADMF is 0
DEEP_ROWS = (10, 20)    # depths up to 60 000


@lru_cache(maxsize=None)
def _inputs(S):
    """depth int32 [P, S, 4], flags int32 [P], admf float64 [P, 4]: records of 2 / 3 / 4 listed alleles, REFMASKED ones among them,
    every fifth row no record, samples without depth, depth on alleles the record does not list."""
    rng = np.random.default_rng(100 + S)
    depth = (rng.integers(0, 40, size=(P, S, 4)) * (rng.random((P, S, 4)) < 0.7)).astype(np.int64)
    depth[rng.random((P, S)) < 0.15] = 0
    for r in DEEP_ROWS:
        depth[r] *= 1500
    depth[DEEP_ROWS[0], 0] = [60000, 60000, 0, 60000]
    flags = np.zeros(P, dtype=np.int64)
    admf = np.full((P, 4), np.nan)
    n_records = 0
    for r in range(P):
        if r % 5 == 2:
            continue
        ref = int(rng.integers(0, 4))
        n_alt = 1 + n_records % 3
        masked = n_alt >= 2 and n_records % 4 == 3
        n_records += 1
        alts = rng.permutation([a for a in range(4) if a != ref])[:n_alt]
        keep = np.zeros(4, dtype=bool)
        keep[alts] = True
        keep[ref] = not masked
        f = np.zeros(4)
        f[keep] = 0.9 * rng.dirichlet(np.ones(int(keep.sum())))
        if r == ZERO_FREQUENCY_ROW:
            f[alts[0]] = 0.0
        desc = np.argsort(f, kind="stable")[::-1]
        flags[r] = sg.record_flag([ref] + [int(a) for a in desc if a != ref], keep)
        admf[r] = f
    listed = sorted({len(sg.enumerated_alleles(f)[0]) + int(sg.enumerated_alleles(f)[1]) for f in flags if f & 1})
    assert listed == [2, 3, 4] and sum(sg.enumerated_alleles(f)[1] for f in flags if f & 1) >= 3
    return depth.astype(np.int32), flags.astype(np.int32), admf


def _ploidy(spec, S):
    return np.resize(np.asarray(spec, dtype=np.int64), S)


NAN = float("nan")
PRIORS = [(None, None), (0.0, None), (0.3, None), (0.0, "ADMF"), (0.3, "ADMF")]
CASES = [(S, (2, 4, 6), F, fr, 0.0024) for S in (3, 70) for F, fr in PRIORS] + [
    (3, (15,), 0.3, "ADMF", 0.0024),
    (3, (15,), None, None, 0.0024),
    (70, (1,), None, None, 0.0024),
    (70, (1, 2, 1), 0.3, "ADMF", 0.0024),
    (70, (2, 4, 6), None, None, 0.0),
    (3, (2, 4, 6), 0.3, "ADMF", 0.0),
    (70, (2, 4, 6), (0.1, NAN, 0.0, 0.5, NAN), "ADMF", 0.0024),   # per sample, NaN = no prior for that sample
    (70, (2, 4, 6), None, "ADMF", 0.0024),                        # frequencies alone: F = 0
]


@pytest.mark.parametrize("S,ploidy,inbreeding,frequencies,error_rate", CASES)
def test_calls_equal_the_definition(S, ploidy, inbreeding, frequencies, error_rate):
    """gpm within rtol 1e-9 of the definition; the same genotype wherever the definition's two highest posteriors differ by more
    than 1e-6 (at most 5 % of the called pairs may be left out for that); the same no-calls; two runs give the same bits."""
    import torch

    from mchap_amd import find_snvs

    depth, flags, admf = _inputs(S)
    k = _ploidy(ploidy, S)
    F = None if inbreeding is None else np.resize(np.asarray(inbreeding, dtype=np.float64), S) if isinstance(inbreeding, tuple) else inbreeding
    want_gt, want_gpm, gap = sg.call(depth, flags, admf, k, F, frequencies, error_rate)
    dev = [torch.from_numpy(x).cuda() for x in (depth, flags, admf)]
    runs = []
    for _ in range(2):
        gt, gpm = find_snvs.genotypes_device(*dev, ploidy=k, inbreeding=F, frequencies=frequencies, error_rate=error_rate)
        assert gt.dtype == torch.int32 and gpm.dtype == torch.float64 and gt.shape == gpm.shape == (P, S)
        runs.append((gt.cpu().numpy(), gpm.cpu().numpy()))
    gt, gpm = runs[0]
    called = want_gt >= 0
    decided = called & (gap > 1e-6)
    rel = np.abs(gpm[called] - want_gpm[called]) / want_gpm[called]
    print("pairs %d called %d undecided %d max relative gpm error %.3g mismatched modes %d" % (
        called.size, called.sum(), (called & ~decided).sum(), rel.max(), (gt[decided] != want_gt[decided]).sum()))
    # rows that are no record, and no-calls
    assert (gt[(flags & 1) == 0] == -1).all() and np.isnan(gpm[(flags & 1) == 0]).all()
    np.testing.assert_array_equal(gt < 0, ~called)
    np.testing.assert_array_equal(np.isnan(gpm), ~called)
    zero = depth.sum(axis=2) == 0
    assert zero.any() and (gt[zero] == -1).all()
    if frequencies == "ADMF":  # a zero frequency is a no-call for every sample that has a prior
        with_prior = ~np.isnan(np.broadcast_to(0.0 if F is None else F, (S,)))
        assert with_prior.any() and (gt[ZERO_FREQUENCY_ROW][with_prior] == -1).all()
    assert called.sum() > 0.5 * ((flags & 1) != 0).sum() * S
    # the calls
    assert np.isfinite(gpm[called]).all() and (gpm[called] > 0).all() and (gpm[called] <= 1.0 + 1e-12).all()
    np.testing.assert_allclose(gpm[called], want_gpm[called], rtol=1e-9, atol=0)
    np.testing.assert_array_equal(gt[decided], want_gt[decided])
    assert (called & ~decided).sum() <= 0.05 * called.sum()
    # reproducible bit for bit
    np.testing.assert_array_equal(runs[1][0], gt)
    np.testing.assert_array_equal(runs[1][1].view(np.int64), gpm.view(np.int64))


def test_deep_rows_keep_a_finite_normaliser():
    """Depth 60 000 on three alleles: every log posterior term is below -1e5 and the mode's probability is still a number."""
    import torch

    from mchap_amd import find_snvs

    depth, flags, admf = _inputs(3)
    lp = sg.log_posterior_terms(depth[DEEP_ROWS[0], 0][sg.enumerated_alleles(flags[DEEP_ROWS[0]])[0]], 2, 0.0024)
    assert lp.max() < -1e5
    gt, gpm = find_snvs.genotypes_device(*[torch.from_numpy(x).cuda() for x in (depth, flags, admf)], ploidy=2)
    assert gt[DEEP_ROWS[0], 0].item() >= 0 and 0.0 < gpm[DEEP_ROWS[0], 0].item() <= 1.0


def test_ploidy_beyond_the_limit_is_refused():
    import torch

    from mchap_amd import _lib, find_snvs

    dev = [torch.from_numpy(x).cuda() for x in _inputs(3)]
    for ploidy in (16, [2, 16, 4]):
        with pytest.raises(NotImplementedError, match="MCHAP_MAX_PLOIDY_DENOVO"):
            find_snvs.genotypes_device(*dev, ploidy=ploidy)
    k = torch.tensor([2, 16, 4], dtype=torch.int32).cuda()
    F = torch.full((3,), float("nan"), dtype=torch.float64).cuda()
    gt = torch.empty((P, 3), dtype=torch.int32).cuda()
    gpm = torch.empty((P, 3), dtype=torch.float64).cuda()
    p = lambda t: t.data_ptr()  # noqa: E731
    rc = _lib.lib().mchap_snv_genotypes_device(p(dev[0]), p(dev[1]), p(dev[2]), P, 3, p(k), p(F), 0, 0.9976, 0.0008, p(gt), p(gpm), None)
    assert rc == _lib.ERR_LIMIT and b"ploidy 16" in _lib.lib().mchap_last_error()
    find_snvs.genotypes_device(*dev, ploidy=15)  # the limit itself is taken


def _source():
    from mchap_amd import application, io

    return application.ReadSource(io.sample_bam_table(BAMS, "SM"), read_group_field="SM")


def _golden_setup():
    from mchap_amd import find_snvs, io

    return find_snvs.read_targets(os.path.join(HERE, "simple.bed")), io.Reference(os.path.join(HERE, "simple.fasta"))


def test_find_snvs_with_calls_writes_the_definitions_records():
    import torch

    from mchap_amd import find_snvs

    targets, reference = _golden_setup()
    source = _source()
    got = list(find_snvs.find_snvs(targets, reference, source, genotypes=dict(ploidy=4)))
    want = []
    for contig, a, b in targets:
        depth = find_snvs.allele_depths(source, contig, a, b)
        ref = find_snvs.bases_to_indices(reference.fetch(contig, a, b).upper())
        flags, admf = find_snvs.filter_device(torch.from_numpy(depth.astype(np.int32)).cuda(), torch.from_numpy(ref))
        flags, admf = flags.cpu().numpy(), admf.cpu().numpy()
        gt, gpm, _ = sg.call(depth, flags, admf, 4)
        rows = np.flatnonzero(flags & 1)
        want += find_snvs.format_records([contig] * len(rows), a + rows, depth[rows], flags[rows], admf[rows], gt_index=gt[rows],
                                         gpm=gpm[rows], ploidy=4)
    assert got == want and len(got) > 3
    fields = [ln.split("\t") for ln in got]
    assert all(f[8] == "GT:GPM:AD" for f in fields)
    assert any(s.split(":")[0].count("/") == 3 and "." not in s.split(":")[0] for f in fields for s in f[9:])
    # per-sample ploidies by name, a prior with the record's ADMF: other calls, the same records otherwise
    mixed = list(find_snvs.find_snvs(targets, reference, source, genotypes=dict(
        ploidy={"SAMPLE1": 2, "SAMPLE2": 4, "SAMPLE3": 6}, inbreeding=0.1, frequencies="ADMF")))
    assert [ln.split("\t")[:9] for ln in mixed] == [f[:9] for f in fields]
    assert all([s.split(":")[0].count("/") for s in ln.split("\t")[9:]] == [1, 3, 5] for ln in mixed)


def test_find_snvs_without_calls_is_unchanged_and_the_program_takes_the_flags():
    from mchap_amd import cli, find_snvs

    targets, reference = _golden_setup()
    golden = [ln.rstrip("\n") for ln in open(os.path.join(HERE, "simple.output.basis.vcf"))]
    plain = list(find_snvs.find_snvs(targets, reference, _source()))
    assert plain == [ln for ln in golden if not ln.startswith("#")]
    base = ["mchap_amd", "find-snvs", "--targets", os.path.join(HERE, "simple.bed"), "--reference", os.path.join(HERE, "simple.fasta"),
            "--bam"] + BAMS
    out = _io.StringIO()
    cli.run(base + ["--call-genotypes", "4"], out)
    lines = out.getvalue().splitlines()
    header = [ln for ln in lines if ln.startswith("#")]
    assert sum(ln.startswith("##FORMAT=<ID=GPM,") for ln in header) == 1 and len(header) == sum(ln.startswith("#") for ln in golden) + 1
    assert [ln for ln in lines if not ln.startswith("#")] == list(find_snvs.find_snvs(targets, reference, _source(), genotypes=dict(ploidy=4)))
    with pytest.raises(ValueError, match="needs --call-genotypes"):
        cli.run(base + ["--call-prior", "ADMF"], _io.StringIO())
