"""The float64 host definition of the SNV genotype posteriors (application.snv_posterior_unit) against the long-double reference
(tests/snv_posterior_reference.py) on every case of tests/estimate_cases.py with M = 5: the envelope the GPU tests' bound is built
on, and the properties of the definition."""
import math

import numpy as np
import pytest

from mchap_amd.application import _genotype_table, _host_log_prior, _logsumexp, _snv_genotype_ranks, snv_posterior_unit
from tests import snv_posterior_reference as ref
from tests.estimate_cases import CASES, build_case

M = 5


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_definition_within_the_envelope(name):
    K, H, _ = CASES[name]
    ha = ref.case_hap_alleles(name, H, M)
    A = [int(ha[:, j].max()) + 1 for j in range(M)]
    assert A[0] == 1 and max(A) == min(H, 4)
    worst = 0.0
    for r in build_case(name):
        for llk, Ku, F in r["units"]:
            for Fu in (F, None):   # (the unit's own F, and the flat prior)
                got = snv_posterior_unit(llk, H, Ku, Fu, r["f"], ha)
                want = ref.snv_posteriors(llk, H, Ku, Fu, r["f"], ha)
                assert got.shape == want.shape == (M, math.comb(max(A) + Ku - 1, Ku))
                worst = max(worst, float(np.max(np.abs(got - want))))
                np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-12)
                for j in range(M):
                    assert np.all(got[j, math.comb(A[j] + Ku - 1, Ku):] == 0.0)
                assert got[0, 0] == pytest.approx(1.0, abs=1e-12)   # the monomorphic column
    print("%s: largest |float64 - long double| = %.3g (envelope %.3g)" % (name, worst, ref.ENVELOPE))
    assert worst <= ref.ENVELOPE


def test_ranks_follow_vcf_order():
    """The closed form of the ranks against the table look-up, four alleles."""
    rng = np.random.default_rng(5)
    for K, H in ((1, 4), (2, 7), (4, 9), (15, 4)):
        g = _genotype_table(H, K)
        alleles = np.concatenate([np.arange(min(H, 4)), rng.integers(0, 4, size=max(0, H - 4))])
        assert np.array_equal(_snv_genotype_ranks(g, alleles), ref.snv_ranks(g, alleles))


def test_distinct_alleles_give_the_haplotype_posterior():
    """M = 1, K = 4, H = 4 with four distinct SNV alleles: the SNV genotypes are the haplotype genotypes."""
    rng = np.random.default_rng(11)
    H = K = 4
    f = rng.dirichlet(np.full(H, 2.0))
    llk = -5.0 * rng.random(math.comb(H + K - 1, K))
    for F in (None, 0.0, 0.3):
        lj = llk + _host_log_prior(_genotype_table(H, K), H, K, F, f)
        p = np.exp(lj - _logsumexp(lj))
        got = snv_posterior_unit(llk, H, K, F, f, np.arange(4).reshape(4, 1))
        assert np.array_equal(got[0], p)


def test_no_finite_genotype_is_nan():
    got = snv_posterior_unit(np.full(10, -np.inf), 4, 2, 0.1, np.full(4, 0.25), np.array([[0, 0], [0, 1], [1, 1], [0, 2]]))
    assert got.shape == (2, 6) and np.all(np.isnan(got))
    want = ref.snv_posteriors(np.full(10, -np.inf), 4, 2, 0.1, np.full(4, 0.25), np.array([[0, 0], [0, 1], [1, 1], [0, 2]]))
    assert ref.within(got, want, 10)[0]
    assert not ref.within(np.zeros((2, 6)), want, 10)[0] and not ref.within(got, np.zeros((2, 6)), 10)[0]
