"""The SNV genotype posteriors of one unit in long double, for the tests of the SNV kernels and of the SNV file
(tests/test_snv_posterior_reference.py, tests/test_gpu_snv_kernels.py, tests/test_gpu_snv_calls.py):
    snv_post[j][s] = sum_g p[g] [s_j(g) = s],   p[g] = exp(llk[g] + lp[g]) / sum_g' exp(llk[g'] + lp[g'])
on tests/estimate_reference.py's genotype table and log prior (sums of logarithms, no lgamma; the prior's constant cancels in p),
with the SNV genotype's rank written out from its definition: the position of the sorted allele tuple in the VCF-ordered table of
the SNV's own alleles.  The float64 host definition that ships, application.snv_posterior_unit, is held to it."""
import math
import zlib

import numpy as np

from tests.estimate_reference import LD, genotype_table, log_prior

# CPU-measured envelope of the float64 host definition against long double on tests/estimate_cases.py's cases with M = 5, the
# largest absolute difference of an entry (tests/test_snv_posterior_reference.py measures, prints and asserts it): 8.75e-13 at
# `K10-H7`, 7.9e-13 at `K15-H6`, 6.7e-13 at `cut-run`, 2.2e-13 at `first-of-KM16`, below 4e-14 at the other cases -- the loss is the prior's: the
# cancellation in lgamma(d + alpha) - lgamma(alpha) at large alpha, which also sets the model evidence's envelope
# (tests/evidence_reference.py)
ENVELOPE = 9e-13
REL = 1e-9
FRACTION_BITS = 62   # the kernel adds p[g] as integers of 62 fraction bits: an entry is off by less than G * 2^-62 on top


def floor(G):
    """FLOOR of the GPU tests' bound |got - want| <= REL |want| + FLOOR: 8 times the envelope -- the project's margin for the
    device's lgamma / exp / log against libm, as tests/evidence_reference.py -- plus the kernel's quantisation term."""
    return 8.0 * ENVELOPE + G * 2.0 ** -FRACTION_BITS


def draw_hap_alleles(rng, H, M):
    """int8 [H, M]: random bases per (haplotype, SNV) as first-appearance indices; column 0 monomorphic, and (M >= 2) column 1
    with min(H, 4) alleles."""
    out = np.zeros((H, M), dtype=np.int8)
    for j in range(1, M):
        bases = rng.integers(0, 4, size=H)
        if j == 1:
            bases[:min(H, 4)] = rng.permutation(4)[:min(H, 4)]
        seen = {}
        for h in range(H):
            out[h, j] = seen.setdefault(int(bases[h]), len(seen))
    return out


def case_hap_alleles(name, H, M):
    return draw_hap_alleles(np.random.default_rng(zlib.crc32(("snv-" + name).encode())), H, M)


def snv_ranks(g, alleles):
    """int64 [G]: the rank of the SNV genotype every genotype implies, looked up in the VCF-ordered table over the SNV's alleles."""
    K = g.shape[1]
    a = np.sort(np.asarray(alleles, dtype=np.int64)[g], axis=1)
    table = genotype_table(int(np.max(alleles)) + 1, K)
    index = {tuple(row): i for i, row in enumerate(table.tolist())}
    return np.array([index[tuple(row)] for row in a.tolist()], dtype=np.int64)


def posterior(llk, H, K, F, f):
    """longdouble [G]: the haplotype-genotype posterior; all NaN where no genotype is finite."""
    g = genotype_table(H, K)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lj = np.asarray(llk, dtype=np.float64).astype(LD)
        if F is not None:
            lj = lj + log_prior(g, H, K, F, f)
        m = np.max(lj)
        if not np.isfinite(m):
            return np.full(len(g), np.nan, dtype=LD)
        p = np.exp(lj - m)
    return p / np.sum(p)


def snv_posteriors(llk, H, K, F, f, hap_alleles, S=None):
    """float64 [M, S]: the definition in long double, rounded at the end.  S: C(A + K - 1, K) for the largest number A of alleles
    of an SNV unless given."""
    ha = np.asarray(hap_alleles).reshape(H, -1)
    if S is None:
        S = math.comb(int(ha.max()) + K, K)
    g = genotype_table(H, K)
    p = posterior(llk, H, K, F, f)
    out = np.zeros((ha.shape[1], S), dtype=LD)
    if np.isnan(p[0]):
        return np.full(out.shape, np.nan)
    for j in range(ha.shape[1]):
        np.add.at(out[j], snv_ranks(g, ha[:, j]), p)
    return out.astype(np.float64)


def within(got, want, G):
    """(every entry within REL |want| + floor(G) -- equal NaNs agree, a NaN where a number is wanted fails --, the largest
    |got - want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or np.any(np.isnan(got) != np.isnan(want)):
        return False, np.inf
    live = ~np.isnan(want)
    err = np.abs(got[live] - want[live])
    return bool(np.all(err <= REL * np.abs(want[live]) + floor(G))), float(err.max()) if err.size else 0.0
