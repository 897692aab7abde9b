"""The float64 host definition of the expected allele depths (application.allele_support_unit) against the long-double reference
(tests/allele_support_reference.py): drawn read tensors -- gaps, all-gap rows, weights 0..5, and error-free reads with cells exactly
0 -- combined with the likelihood tables of tests/estimate_cases.py and with likelihoods formed from the reads themselves.  The
envelope the GPU tests' bound is built on, and the invariants of the definition.  CPU only."""
import zlib

import numpy as np
import pytest

from mchap_amd.application import allele_support_unit
from tests import allele_support_reference as ref
from tests.estimate_cases import CASES, build_case

A = 3
R = 9


def positions(H):
    """SNVs that give at least 2 H haplotypes over A alleles, 4 or more."""
    m = 4
    while A ** m < 2 * H:
        m += 1
    return m


def case_inputs(name):
    """[(dists, counts, haps, llk, K, F, f, own)] of a case: every unit of tests/estimate_cases.py's records with a drawn read tensor
    -- its table (own False) --, and per record the likelihoods of drawn reads themselves, noisy and error-free (own True)."""
    K, H, _ = CASES[name]
    rng = np.random.default_rng(zlib.crc32(("support-" + name).encode()))
    haps = ref.draw_haplotypes(rng, H, positions(H), A)
    out = []
    for r in build_case(name):
        for u, (llk, Ku, F) in enumerate(r["units"][:3 if H <= 100 else 1]):   # (500 haplotypes: one table, the reference is a loop)
            dists, counts = ref.draw_reads(rng, haps, R, A, error_free=(u == 1))
            out.append((dists, counts, haps, llk, Ku, F, r["f"], False))
        for error_free in ((False, True) if H <= 100 else (True,)):
            dists, counts = ref.draw_reads(rng, haps, R, A, error_free=error_free)
            out.append((dists, counts, haps, ref.likelihoods(dists, counts, haps, K), K, r["units"][error_free][2], r["f"], True))
    return out


def deviation(got, want, weight):
    """The largest |float64 - long double|: of depth over the unit's read weight, and of an entry of a read's row (weight 1)."""
    if np.all(np.isnan(want[0])):   # (no finite genotype under this prior: NaN on both sides)
        assert np.all(np.isnan(got[0])) and np.all(np.isnan(got[1])) and np.all(np.isnan(want[1]))
        return 0.0
    assert not np.any(np.isnan(want[0])) and not np.any(np.isnan(got[0]))
    return max(float(np.max(np.abs(got[0] - want[0]))) / weight, float(np.max(np.abs(got[1] - want[1]))))


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_definition_within_the_envelope(name):
    K, H, _ = CASES[name]
    worst = 0.0
    for dists, counts, haps, llk, Ku, F, f, own in case_inputs(name):
        N = float(counts.sum())
        for Fu in ((F, None) if H <= 100 else (F,)):   # (the unit's own F, and the flat prior)
            got = allele_support_unit(dists, counts, haps, llk, Ku, Fu, f)
            want = ref.support(dists, counts, haps, llk, Ku, Fu, f)
            assert got[0].shape == want[0].shape == (H,) and got[1].shape == want[1].shape == (R, H)
            worst = max(worst, deviation(got, want, N))
            depth, post = got
            if np.isnan(depth[0]):
                continue
            assert np.all(post[counts == 0] == 0.0) and np.all(post >= 0.0)
            assert np.array_equal(depth, (counts[counts > 0, None] * post[counts > 0]).sum(axis=0))
            if own:
                # likelihoods of these very reads: a genotype with p > 0 explains every read with a weight, so every such row sums
                # to 1 and the depths to the read weight
                np.testing.assert_allclose(post[counts > 0].sum(axis=1), 1.0, rtol=0, atol=1e-12)
                np.testing.assert_allclose(depth.sum(), N, rtol=1e-12)
            else:
                assert np.all(post.sum(axis=1) <= 1.0 + 1e-12)   # (a foreign table: a pair with D = 0 contributes 0)
    print("%s: largest |float64 - long double| per unit of read weight = %.3g (envelope %.3g, set by %s)" % (
        name, worst, ref.ENVELOPE, ref.ENVELOPE_CASE))
    assert worst <= ref.ENVELOPE


def test_an_all_gap_row_gives_the_posterior_mean_frequencies():
    from mchap_amd.application import _genotype_table, _host_log_prior, _logsumexp

    H, K, M = 5, 4, 4
    rng = np.random.default_rng(3)
    haps = ref.draw_haplotypes(rng, H, M, A)
    dists, counts = ref.draw_reads(rng, haps, R, A)
    counts[3] = 2
    assert np.all(np.isnan(dists[3]))
    llk = ref.likelihoods(dists, counts, haps, K)
    f = rng.dirichlet(np.full(H, 2.0))
    for F in (None, 0.0, 0.3):
        g = _genotype_table(H, K)
        lj = llk + _host_log_prior(g, H, K, F, f)
        p = np.exp(lj - _logsumexp(lj))
        freq = np.array([(p * (g == h).sum(axis=1)).sum() / K for h in range(H)])
        _, post = allele_support_unit(dists, counts, haps, llk, K, F, f)
        np.testing.assert_allclose(post[3], freq, rtol=0, atol=1e-14)
        np.testing.assert_allclose(ref.support(dists, counts, haps, llk, K, F, f)[1][3], freq, rtol=0, atol=1e-14)


def test_zero_weights_and_no_finite_genotype():
    H, K, M = 4, 2, 3
    rng = np.random.default_rng(8)
    haps = ref.draw_haplotypes(rng, H, M, A)
    dists, counts = ref.draw_reads(rng, haps, R, A)
    llk = ref.likelihoods(dists, counts, haps, K)
    f = np.full(H, 0.25)
    depth, post = allele_support_unit(dists, np.zeros(R, dtype=np.int64), haps, llk, K, 0.1, f)
    assert np.all(depth == 0.0) and np.all(post == 0.0)
    want = ref.support(dists, np.zeros(R, dtype=np.int64), haps, llk, K, 0.1, f)
    assert np.all(want[0] == 0.0) and np.all(want[1] == 0.0)
    dead = np.full(len(llk), -np.inf)
    depth, post = allele_support_unit(dists, counts, haps, dead, K, 0.1, f)
    assert depth.shape == (H,) and post.shape == (R, H) and np.all(np.isnan(depth)) and np.all(np.isnan(post))
    want = ref.support(dists, counts, haps, dead, K, 0.1, f)
    assert ref.within(depth, want[0], float(counts.sum()))[0] and ref.within(post, want[1], 1.0)[0]
    assert not ref.within(np.zeros(H), want[0], 1.0)[0] and not ref.within(depth, np.zeros(H), 1.0)[0]
    # counts None: every weight 1
    d1 = allele_support_unit(dists, None, haps, llk, K, None, f)[0]
    assert np.array_equal(d1, allele_support_unit(dists, np.ones(R, dtype=np.int64), haps, llk, K, None, f)[0])
