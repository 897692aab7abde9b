"""The long-double reference of the model evidence (tests/evidence_reference.py) anchored on the CPU: the priors it sums over are
normalised (an all-zero likelihood table has evidence 0), and the envelope of the kernels' float64 lgamma form against it, by F,
on the inputs the GPU tests use (tests/estimate_cases.py)."""
import zlib
from math import comb

import numpy as np
import pytest

from tests import estimate_cases as cases
from tests import evidence_reference as ref

GRID_F = tuple(sorted(set(cases.F_VALUES) | {1e-3}))   # the F values the envelope is stated for


def _rows(name):
    """The frequency rows of a case, one per variant the case's H allows: [(variant, f)]."""
    K, H, _ = cases.CASES[name]
    rng = np.random.default_rng(zlib.crc32(b"evidence rows " + name.encode()))
    return [(v, cases.frequency_row(rng, H, v)) for v in cases.variants_for(H)]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_priors_sum_to_one(name):
    """An all-zero table: evidence = log sum_g prior(g) = 0, for every F of estimate_cases.F_VALUES, the flat prior, and every
    frequency variant."""
    K, H, _ = cases.CASES[name]
    zeros = np.zeros(comb(H + K - 1, K))
    worst = 0.0
    for variant, f in _rows(name):
        for F in cases.F_VALUES + (None,):
            for form in (ref.evidence, ref.evidence_lgamma):
                ev = form(zeros, H, K, F, f)
                worst = max(worst, abs(ev))
                assert abs(ev) <= (1e-14 if form is ref.evidence else ref.floor(F)), (name, variant, F, form.__name__, ev)
    print("%s: largest |evidence| of an all-zero table %.3g" % (name, worst))


def test_the_envelope_of_the_lgamma_form():
    """|float64 lgamma form - long double| over every table of every case, at every F of the grid: measured, printed, and held to
    the envelope the GPU tests' FLOOR is 8 times of."""
    worst = {F: 0.0 for F in GRID_F + (None,)}
    largest = 0.0
    for name, (K, H, _) in cases.CASES.items():
        for rec in cases.build_case(name):
            for llk, _, _ in rec["units"]:
                for F in GRID_F + (None,):
                    want, got = ref.evidence(llk, H, K, F, rec["f"]), ref.evidence_lgamma(llk, H, K, F, rec["f"])
                    assert np.isfinite(want) and np.isfinite(got), (name, F, want, got)
                    worst[F] = max(worst[F], abs(got - want))
                    largest = max(largest, abs(want))
    for F in GRID_F + (None,):
        print("F = %s: worst |lgamma form - long double| %.3g (envelope %.3g)" % (F, worst[F], ref.envelope(F)))
    print("largest |evidence| %.6g" % largest)
    for F in GRID_F + (None,):
        assert worst[F] <= ref.envelope(F), (F, worst[F])


def test_the_constants_against_brute_force():
    """The normalised prior of a small shape against the definition written out: the multinomial and the Dirichlet-multinomial pmf
    from products of ratios, in long double."""
    from tests.estimate_reference import LD, genotype_table, log_prior

    H, K = 3, 4
    f = np.array([0.5, 0.3, 0.2])
    g = genotype_table(H, K)
    for F in (0.0, 0.1):
        lp = log_prior(g, H, K, F, f) + ref.log_prior_constant(H, K, F, f)
        for i, row in enumerate(g):
            d = np.bincount(row, minlength=H)
            if F == 0.0:
                p = LD(24)
                for h in range(H):
                    p *= LD(f[h]) ** int(d[h]) / LD(np.prod(np.arange(1, d[h] + 1)))
            else:
                alpha = f.astype(LD) * ((LD(1) - LD(F)) / LD(F))
                p = LD(24)
                for j in range(K):
                    p /= np.sum(alpha) + j
                for h in range(H):
                    for j in range(d[h]):
                        p *= (alpha[h] + j) / LD(j + 1)
            assert abs(float(np.exp(lp[i]) - p)) < 1e-17, (F, row, float(np.exp(lp[i])), float(p))
    assert abs(ref.evidence(np.zeros(len(g)), H, K, None, f)) < 1e-18


def test_a_zero_frequency_masks_its_genotypes():
    H, K = 4, 3
    f = np.array([0.0, 0.5, 0.25, 0.25])
    from tests.estimate_reference import genotype_table

    g = genotype_table(H, K)
    llk = np.where(np.any(g == 0, axis=1), 0.0, -np.inf)   # only genotypes holding the masked allele are finite
    for F in (0.0, 0.1):
        assert ref.evidence(llk, H, K, F, f) == -np.inf and ref.evidence_lgamma(llk, H, K, F, f) == -np.inf
    assert ref.evidence(llk, H, K, None, f) > -np.inf   # (the flat prior knows no frequencies)
