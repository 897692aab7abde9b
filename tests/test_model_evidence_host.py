"""call-exact --model-evidence on the host: the definition (application.model_evidence_host on the oracle) against the long-double
reference (tests/evidence_reference.py) on a small block, the accumulator's sums, counts and skipping rule, and the table's text.
CPU only."""
import numpy as np
import pytest

from mchap_amd import application
from tests import evidence_reference as ref
from tests.estimate_units import fresh, make_record, per_sample, samples_of

PLOIDIES = (2, 4, 4, 2)          # the samples' own
INBREEDING = (0.01, 0.3, 0.3, 0.01)
READS = (12, 9, 0, 15)           # S2 has no reads
CAND_K, CAND_F = (2, 4), (0.01, 0.3)


@pytest.fixture(scope="module")
def oracle():
    from tests.replay_call_exact import OracleBackend

    return OracleBackend()


def _block():
    """Six records x four samples, H from 2 to 6 (one masked reference, non-flat rows), and a record with one haplotype."""
    rng = np.random.default_rng(29)
    units = []
    for i, (H, M) in enumerate([(2, 2), (3, 2), (4, 3), (1, 2), (6, 3), (5, 3)]):
        f0 = rng.dirichlet(np.full(H, 2.0))
        units.append(make_record(rng, H, M, PLOIDIES, READS, masked=(i == 2), f0=f0, name="r%d" % i))
    units[3]["needs_kernel"] = False   # (one haplotype: one genotype with probability 1, as _exact_units marks it)
    return units


def _reference_sums(units, oracle, cands):
    """{sample: long-double-reference sums over the records in record order, float64 accumulation}."""
    sums = {s: np.zeros(len(cands)) for s in samples_of(units)}
    for unit in units:
        if not unit["needs_kernel"]:
            continue
        locus = unit["locus"]
        H = len(locus.haplotypes)
        for s, sr in unit["reads"].items():
            ev = np.zeros(len(cands))
            for c, (K, F) in enumerate(cands):
                llk = np.asarray(oracle.genotype_likelihoods(sr["dists"], K, locus.haplotypes, read_counts=sr["counts"]), dtype=np.float64)
                ev[c] = ref.evidence(llk, H, K, F, locus.frequencies)
            sums[s] = sums[s] + ev
    return sums


def test_the_definition_against_long_double(oracle):
    units = _block()
    samples = samples_of(units)
    cands = [(K, F) for K in CAND_K for F in CAND_F]
    acc = application.ModelEvidence(samples, CAND_K, CAND_F)
    got = acc.add_block(fresh(units), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    assert acc.candidates == {s: cands for s in samples}
    assert sorted({ri for ri, _ in got}) == [0, 1, 2, 4, 5]           # the record with one haplotype is not counted
    want = _reference_sums(units, oracle, cands)
    for s in samples:
        assert acc.records[s] == 5 and acc.skipped[s] == 0
        for c, (K, F) in enumerate(cands):
            ok, err = ref.within(acc.sums[s][c], want[s][c], F)
            print("%s K=%d F=%g: %.9f (reference %.9f, |difference| %.3g)" % (s, K, F, acc.sums[s][c], want[s][c], err))
            assert ok, (s, K, F, acc.sums[s][c], want[s][c])
    assert np.all(acc.sums["S2"] == 0.0)                               # a sample without reads contributes exactly 0
    assert all(np.all(got[(ri, "S2")] == 0.0) for ri in (0, 1, 2, 4, 5))
    assert all(np.all(acc.sums[s] < 0.0) for s in ("S0", "S1", "S3"))
    # the sums are the per-record values added in record order
    for s in samples:
        run = np.zeros(len(cands))
        for ri in (0, 1, 2, 4, 5):
            run = run + got[(ri, s)]
        assert np.array_equal(run, acc.sums[s])
    rows = acc.table()
    assert [r["configured"] for r in rows if r["sample"] == "S0"] == [1, 0, 0, 0]
    assert [r["configured"] for r in rows if r["sample"] == "S1"] == [0, 0, 0, 1]
    for s in samples:
        mine = [r for r in rows if r["sample"] == s]
        assert max(r["delta"] for r in mine) == 0.0 and all(r["delta"] <= 0.0 for r in mine)


def test_the_flat_prior_and_the_defaults(oracle):
    units = _block()
    samples = samples_of(units)
    acc = application.ModelEvidence(samples, CAND_K)
    acc.add_block(fresh(units), per_sample(PLOIDIES), lambda s: None, backend=oracle)
    cands = [(2, None), (4, None)]
    assert acc.candidates == {s: cands for s in samples}
    want = _reference_sums(units, oracle, cands)
    for s in samples:
        for c in range(2):
            ok, err = ref.within(acc.sums[s][c], want[s][c], None)
            assert ok, (s, c, acc.sums[s][c], want[s][c], err)
    # defaults: the sample's own pair alone; duplicates among the candidates are dropped, the order given is kept
    own = application.ModelEvidence(samples)
    own.add_block(fresh(units), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    assert own.candidates == {s: [(PLOIDIES[i], INBREEDING[i])] for i, s in enumerate(samples)}
    assert all(r["configured"] == 1 and r["delta"] == 0.0 for r in own.table())
    dup = application.ModelEvidence(samples, (4, 2, 4), (0.3, 0.3, 0.0))
    dup.add_block(fresh(units), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    assert dup.candidates["S0"] == [(4, 0.3), (4, 0.0), (2, 0.3), (2, 0.0)]
    with pytest.raises(ValueError, match="flat genotype prior"):
        application.ModelEvidence(samples, None, (0.1,)).add_block(fresh(units), per_sample(PLOIDIES), lambda s: None, backend=oracle)
    for bad in ((0.1, 1.0), (-0.1,), (float("nan"),), (float("inf"),)):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            application.ModelEvidence(samples, None, bad)
    with pytest.raises(ValueError, match="ploidies"):
        application.ModelEvidence(samples, (0, 2))


def test_a_unit_one_candidate_cannot_take_is_skipped_for_all(oracle):
    """H = 200 at the candidate K = 15 has 2^62 genotypes or more: the record is SKIPPED for every row of every sample and left
    out of all sums -- those of ploidy 2 too; with ploidy 2 as the only candidate it is counted."""
    from math import comb

    assert comb(200 + 15 - 1, 15) >= 1 << 62
    rng = np.random.default_rng(31)
    small = _block()[:2]
    big = make_record(rng, 200, 8, PLOIDIES, (3, 2, 0, 2), name="big")
    units = [small[0], big, small[1]]
    samples = samples_of(units)
    acc = application.ModelEvidence(samples, (2, 15), (0.3,))
    got = acc.add_block(fresh(units), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    assert all(got[(1, s)] is None for s in samples) and all(got[(ri, s)] is not None for ri in (0, 2) for s in samples)
    without = application.ModelEvidence(samples, (2, 15), (0.3,))
    without.add_block(fresh([small[0], small[1]]), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    for s in samples:
        assert acc.records[s] == 2 and acc.skipped[s] == 1
        assert np.array_equal(acc.sums[s], without.sums[s])
    assert all(r["skipped"] == 1 and r["records"] == 2 for r in acc.table())
    assert acc.records_seen == 3
    assert all(u["invalid"] is None for u in units)                  # (never FILTER=LIMIT)
    # a ploidy beyond the library skips the same way
    beyond = application.ModelEvidence(samples, (2, 16), (0.3,))
    beyond.add_block(fresh(small), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    assert all(beyond.skipped[s] == 2 and beyond.records[s] == 0 and np.all(beyond.sums[s] == 0.0) for s in samples)
    # ploidy 2 alone takes the large record
    two = application.ModelEvidence(samples, (2,), (0.3,))
    two.add_block(fresh([big]), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    assert all(two.records[s] == 1 and two.skipped[s] == 0 for s in samples)


def test_which_units_can_be_evaluated():
    """application._evidence_evaluable, the screen both the definition and the device path apply unit by unit."""
    from math import comb

    ok = application._evidence_evaluable
    assert ok(6, [(2, 0.1), (4, 0.0)]) and ok(6, [(15, None)]) and not ok(6, [(2, 0.1), (16, 0.1)]) and not ok(6, [(0, None)])
    assert not ok(200, [(2, 0.1), (15, 0.1)]) and ok(200, [(2, 0.1)])
    # the prior tables of one grid point beyond the evidence kernel's LDS (K = 2: from H = 4030); the flat prior has no tables
    assert ok(4029, [(2, 0.1)]) and not ok(4030, [(2, 0.1)]) and not ok(4030, [(2, None), (2, 0.0)]) and ok(4030, [(2, None)])
    # one unit's likelihoods against the device budget
    need = application._exact_unit_bytes(comb(6 + 4 - 1, 4), 8)
    assert ok(6, [(2, 0.1), (4, 0.1)], need) and not ok(6, [(2, 0.1), (4, 0.1)], need - 1) and ok(6, [(2, 0.1)], need - 1)


TABLE = """\
# mchap_amd call-exact model evidence; frequencies: tag AFP; records: 6
SAMPLE\tPLOIDY\tINBREEDING\tRECORDS\tSKIPPED\tLOG_EVIDENCE\tDELTA\tCONFIGURED
S0\t2\t0.01\t5\t0\t-51.197601\t0.000000\t1
S0\t2\t0.3\t5\t0\t-52.286918\t-1.089317\t0
S0\t4\t0.01\t5\t0\t-55.586277\t-4.388676\t0
S0\t4\t0.3\t5\t0\t-53.109931\t-1.912330\t0
S1\t2\t0.01\t5\t0\t-47.861200\t-2.551008\t0
S1\t2\t0.3\t5\t0\t-49.588751\t-4.278559\t0
S1\t4\t0.01\t5\t0\t-45.310191\t0.000000\t0
S1\t4\t0.3\t5\t0\t-46.464746\t-1.154555\t1
S2\t2\t0.01\t5\t0\t0.000000\t0.000000\t0
S2\t2\t0.3\t5\t0\t0.000000\t0.000000\t0
S2\t4\t0.01\t5\t0\t0.000000\t0.000000\t0
S2\t4\t0.3\t5\t0\t0.000000\t0.000000\t1
S3\t2\t0.01\t5\t0\t-45.165387\t0.000000\t1
S3\t2\t0.3\t5\t0\t-45.327189\t-0.161802\t0
S3\t4\t0.01\t5\t0\t-54.194592\t-9.029205\t0
S3\t4\t0.3\t5\t0\t-49.085391\t-3.920003\t0
"""


def test_the_table_text(oracle, tmp_path):
    units = _block()
    samples = samples_of(units)
    acc = application.ModelEvidence(samples, CAND_K, CAND_F, frequency_source="tag AFP")
    # two blocks: the sums run on
    acc.add_block(fresh(units[:3]), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    acc.add_block(fresh(units[3:]), per_sample(PLOIDIES), per_sample(INBREEDING), backend=oracle)
    path = tmp_path / "evidence.tsv"
    acc.write(str(path))
    text = path.read_text()
    print(text)
    assert text == acc.text() == TABLE
