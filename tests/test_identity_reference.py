"""The float64 host definition of the identity evidence -- application.identity_unit -- against the long-double restatement in
plain loops (tests/identity_reference.py), and the properties of the definition: r = sum post_i post_j / pi, symmetry, a copy of
a sample scores above 0, rows peaked on different genotypes score log e, the 1e-290 clause, the exact 0 of a sample without
reads and of a single haplotype, a zero frequency.  CPU only."""
from math import comb, log

import numpy as np
import pytest

from mchap_amd import application
from tests import identity_reference as ref


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_host_definition_against_long_double():
    worst, at = 0.0, None
    for K, H in ref.SHAPES:
        G = comb(H + K - 1, K)
        for n in (1, 3, 5):
            llk, reads, fr = ref.draw_case(K, H, n)
            for F in ref.PRIORS:
                for e in (0.0, 0.01):
                    for r in range(3):
                        lp = ref.log_prior(K, H, F, fr[r])
                        got = application.identity_unit(llk[r], lp, e, reads[r])
                        want = ref.lbf(llk[r], lp, e, reads[r])
                        ok, err = ref.within(got, want, G)
                        assert ok, (K, H, n, F, e, r, err)
                        assert np.all(np.isnan(np.diag(got))) and got.shape == (n, n)
                        if err > worst:
                            worst, at = err, (K, H, n, F, e, r)
    print("largest |float64 - long double| of a term: %.3g at %r" % (worst, at))
    assert worst <= 1e-13   # (measured 1.33e-15: the terms are of one sign, the sums lose nothing)


@pytest.fixture(scope="module")
def drawn():
    K, H = 4, 4
    rng = np.random.default_rng(11)
    f = rng.dirichlet(np.full(H, 2.0))
    return K, H, f, -rng.exponential(4.0, size=(6, comb(H + K - 1, K)))


@pytest.mark.parametrize("F", ref.PRIORS)
def test_r_is_the_sum_of_posterior_products_over_the_prior_and_is_symmetric(drawn, F):
    K, H, f, llk = drawn
    lp = ref.log_prior(K, H, F, f)
    post = np.stack([application._unit_posterior(row, H, K, F, f)[0] for row in llk])
    r = np.einsum("ig,jg->ij", post, post / np.exp(lp))
    for e in (0.0, 0.01, 0.5, 1.0):
        got = application.identity_unit(llk, lp, e)
        off = ~np.eye(len(llk), dtype=bool)
        assert np.allclose(got[off], np.log((1 - e) * r + e)[off], rtol=1e-10, atol=1e-12)
        assert np.array_equal(bits(got[off]), bits(got.T[off]))
    assert np.all(application.identity_unit(llk, lp, 1.0)[off] == 0.0)


def test_a_copy_scores_above_zero_and_peaked_rows_score_log_e(drawn):
    K, H, f, llk = drawn
    G = llk.shape[1]
    lp = ref.log_prior(K, H, 0.3, f)
    both = np.vstack([llk, llk[:1]])
    assert application.identity_unit(both, lp, 0.01)[0, 6] > 0.0
    # two rows each certain of another genotype: r is 0 to rounding, the term log e
    peaked = np.full((2, G), -60.0)
    peaked[0, 3], peaked[1, 17] = 0.0, 0.0
    for e in (0.01, 0.2):
        assert abs(application.identity_unit(peaked, lp, e)[0, 1] - log(e)) <= 1e-12
    # ... and both certain of one genotype: 1 / pi(g), bounded by -log pi(g)
    peaked[1] = peaked[0]
    assert abs(application.identity_unit(peaked, lp, 0.0)[0, 1] + lp[3]) <= 1e-9


def test_the_clause(drawn):
    K, H, f, _ = drawn
    G = comb(H + K - 1, K)
    lp = ref.log_prior(K, H, None, f)
    for apart in (400.0, 2000.0):    # a scaled sum of about 2 exp(-400) = 4e-174, above 1e-290; 2 exp(-2000) is below
        peaked = np.full((2, G), -apart)
        peaked[0, 0], peaked[1, G - 1] = 0.0, 0.0
        at0 = application.identity_unit(peaked, lp, 0.0)[0, 1]
        at1 = application.identity_unit(peaked, lp, 0.01)[0, 1]
        if apart > 700:
            assert at0 == -np.inf and bits(at1) == bits(np.log(0.01))
            assert ref.lbf(peaked, lp, 0.0)[0, 1] == -np.inf and bits(ref.lbf(peaked, lp, 0.01)[0, 1]) == bits(np.log(0.01))
        else:
            assert np.isfinite(at0) and at0 < -390.0 and abs(at1 - log(0.01)) <= 1e-12
    # just either side of the threshold: rows certain of different genotypes that share one genotype at -d / 2 each
    for d, cut in ((660.0, False), (672.0, True)):
        rows = np.full((2, G), -np.inf)
        rows[0, 0], rows[1, 1] = 0.0, 0.0
        rows[0, 2], rows[1, 2] = -d / 2, -d / 2        # S = exp(-d): 2.3e-287 at 660, 1.4e-292 at 672
        got = application.identity_unit(rows, lp, 0.0)[0, 1]
        assert (got == -np.inf) if cut else (np.isfinite(got) and got < -600.0)
        assert ref.within(np.array([got]), np.array([ref.lbf(rows, lp, 0.0)[0, 1]]), G)[0]


def test_a_sample_without_reads_and_a_single_haplotype_are_exactly_zero(drawn):
    K, H, f, llk = drawn
    lp = ref.log_prior(K, H, 0.0, f)
    blank = llk.copy()
    blank[2] = np.nan                                  # (not to be looked at)
    got = application.identity_unit(blank, lp, 0.01, reads=[1, 1, 0, 1, 1, 1])
    full = application.identity_unit(llk, lp, 0.01)
    off = [i for i in range(6) if i != 2]
    assert np.array_equal(bits(got[2, off]), bits(np.zeros(5))) and np.array_equal(bits(got[off, 2]), bits(np.zeros(5)))
    assert np.array_equal(bits(got[np.ix_(off, off)]), bits(full[np.ix_(off, off)]))
    # its likelihoods, were they looked at, are all 0: r is 1 to rounding
    blank[2] = 0.0
    assert np.all(np.abs(application.identity_unit(blank, lp, 0.01)[2, off]) <= 1e-12)
    # a sample without a finite genotype: NaN in its row and column, also against the sample without reads
    blank[4] = -np.inf
    got = application.identity_unit(blank, lp, 0.01, reads=[1, 1, 0, 1, 1, 1])
    assert np.all(np.isnan(got[4])) and np.all(np.isnan(got[:, 4])) and got[2, 0] == 0.0 and got[0, 1] == full[0, 1]
    # one haplotype: one genotype, pi = 1, r = 1
    one = application.identity_unit(np.array([[-3.0], [-7.5], [-1.0]]), np.zeros(1), 0.01)
    assert np.array_equal(bits(one[~np.eye(3, dtype=bool)]), bits(np.zeros(6)))
    assert application.identity_unit(np.array([[-3.0, -1.0]]), np.log([0.5, 0.5]), 0.01).shape == (1, 1)


def test_a_zero_frequency():
    K, H = 2, 3
    f = np.array([0.6, 0.0, 0.4])
    rng = np.random.default_rng(3)
    llk = -rng.exponential(4.0, size=(3, comb(H + K - 1, K)))
    for F in (0.0, 0.3):
        lp = ref.log_prior(K, H, F, f)
        assert np.sum(lp == -np.inf) == 3                # 0/1, 1/1, 1/2
        got = application.identity_unit(llk, lp, 0.01)
        assert np.all(np.isfinite(got[~np.eye(3, dtype=bool)]))
        ok, err = ref.within(got, ref.lbf(llk, lp, 0.01), len(lp))
        assert ok, err
        # a sample whose only possible genotypes the prior excludes has no finite genotype
        only = np.full((2, len(lp)), -np.inf)
        only[0, np.flatnonzero(lp == -np.inf)[0]] = -1.0
        only[1, 0] = -1.0
        assert np.isnan(application.identity_unit(only, lp, 0.01)[0, 1])
