"""The model evidence of one unit in long double, for the tests of the evidence kernels and of the program's table
(tests/test_evidence_reference.py, tests/test_model_evidence_host.py, tests/test_gpu_evidence_kernels.py,
tests/test_gpu_model_evidence.py): log sum_g P(g | K, F, f) exp(llk[g]) with the prior of tests/estimate_reference.py -- sums of
logarithms, no lgamma anywhere -- and the constants that file's "up to a constant" leaves out:
    F > 0:  log K! - sum_{i < K} log(sum_alpha + i)      (Dirichlet-multinomial, alpha = f (1 - F) / F)
    F = 0:  log K!                                        (multinomial)
    flat:   -log G                                        (F None: the uniform prior over the G genotypes)
The kernels' own form in float64 (math.lgamma tables, calling_log_prior) stands beside it -- the program's host definition,
application._host_log_prior: what separates the two is the loss of the formula, not of an implementation."""
import math

import numpy as np

from tests.estimate_reference import LD, genotype_table, log_prior

# CPU-measured envelope of the float64 lgamma form against long double on tests/estimate_cases.py's cases, absolute, by F
# (tests/test_evidence_reference.py measures, prints and asserts it), and the bound of the GPU tests:
# |got - want| <= REL * |want| + FLOOR with FLOOR 8 times the envelope -- the margin covers the device's lgamma / exp / log against
# libm.
ENVELOPE = {0.0: 3e-14, 1e-4: 1.6e-11, 1e-3: 2.3e-12, 0.1: 2.3e-12, 0.5: 2.3e-12, 0.99: 3e-14}
ENVELOPE_FLAT = 3e-14
REL = 1e-9


def envelope(F):
    """The envelope for an F of the grid: the table's entry, or for an F between entries the larger of its neighbours'."""
    if F is None:
        return ENVELOPE_FLAT
    if F in ENVELOPE:
        return ENVELOPE[F]
    keys = sorted(ENVELOPE)
    assert keys[1] <= F <= keys[-1], "no envelope measured for 0 < F < 1e-4"
    lo = max(k for k in keys if k <= F)
    hi = min(k for k in keys if k >= F)
    return max(ENVELOPE[lo], ENVELOPE[hi])


def floor(F):
    return 8.0 * envelope(F)


def log_prior_constant(H, K, F, f):
    """longdouble: what log_prior leaves out, so that the prior sums to 1 over the genotypes."""
    log_kfact = np.sum(np.log(np.arange(1, K + 1).astype(LD))) if K > 1 else LD(0)
    if F is None:
        return -np.log(LD(math.comb(H + K - 1, K)))
    if F > 0:
        alpha = np.asarray(f, dtype=np.float64).astype(LD) * ((LD(1) - LD(F)) / LD(F))
        sa = np.sum(alpha)
        return log_kfact - np.sum(np.log(sa + np.arange(K).astype(LD)))
    return log_kfact


def evidence(llk, H, K, F, f):
    """float64: log sum_g prior(g) exp(llk[g]) of one unit in long double, rounded at the end; -inf where no genotype is finite."""
    g = genotype_table(H, K)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lj = np.asarray(llk, dtype=np.float64).astype(LD)
        if F is not None:
            lj = lj + log_prior(g, H, K, F, f)
        m = np.max(lj)
        if not np.isfinite(m):
            return -np.inf
        return float(m + np.log(np.sum(np.exp(lj - m))) + log_prior_constant(H, K, F, f))


def log_prior_lgamma(g, H, K, F, f):
    """float64 [G]: the normalised log prior the way the kernels form it (calling_log_prior on the tables of exact_setup): the
    host definition that ships, application._host_log_prior -- the envelope is measured on it, not on a copy."""
    from mchap_amd.application import _host_log_prior

    return _host_log_prior(g, H, K, F, f)


def evidence_lgamma(llk, H, K, F, f):
    """float64: the same quantity in float64 throughout, in the kernels' form."""
    g = genotype_table(H, K)
    with np.errstate(invalid="ignore", over="ignore"):
        lj = np.asarray(llk, dtype=np.float64) + log_prior_lgamma(g, H, K, F, f)
        m = np.max(lj)
        if not np.isfinite(m):
            return -np.inf
        return float(m + np.log(np.sum(np.where(lj > -np.inf, np.exp(lj - m), 0.0))))


def within(got, want, F):
    """(|got - want| <= REL |want| + FLOOR(F) -- equal infinities agree, a NaN fails --, |got - want|)."""
    if np.isinf(want) or np.isinf(got):
        return bool(got == want), 0.0 if got == want else np.inf
    err = abs(float(got) - float(want))
    return bool(err <= REL * abs(float(want)) + floor(F)), err
