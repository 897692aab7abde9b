"""Shared helpers for the tests (not part of the product)."""
import numpy as np
from scipy import stats as _stats


def beta_break_table(n_pos, alpha=1.0, beta=3.0):
    """Row m = Beta(alpha, beta) CDF increments over m het bases (what DenovoMCMC computes with scipy,
    reference assemble/mcmc.py:429-452), zero padded to n_pos columns."""
    tab = np.zeros((n_pos + 1, max(n_pos, 1)))
    dist = _stats.beta(alpha, beta)
    for m in range(1, n_pos + 1):
        pts = np.arange(1, m + 1) / m
        probs = dist.cdf(pts)
        probs[1:] = probs[1:] - probs[:-1]
        tab[m, :m] = probs
    return tab


def lexsort_rows(g):
    """Canonical haplotype order of one genotype [K, M] (position 0 most significant)."""
    g = np.asarray(g)
    return g[np.lexsort(np.flip(g, axis=-1).T)]


def assert_same_posterior(got_genotypes, got_probs, exp_genotypes, exp_probs, rtol=1e-15):
    """Posterior lists (probability descending) are equal: the same probabilities in the same order, and the same
    genotypes -- in the same order where the probabilities differ, as the same SET inside a run of tied probabilities.
    The reference orders with np.flip(np.argsort(probs)) (assemble/classes.py:316-325); numpy's default argsort is not
    stable (the AVX-512 sort of numpy 2.x reorders ties even among 4 elements), so the order inside a tie is not
    defined by the reference.  This build's rule (descending first appearance) is pinned separately."""
    got_genotypes, exp_genotypes = np.asarray(got_genotypes), np.asarray(exp_genotypes)
    got_probs, exp_probs = np.asarray(got_probs, float), np.asarray(exp_probs, float)
    assert got_genotypes.shape == exp_genotypes.shape
    np.testing.assert_allclose(got_probs, exp_probs, rtol=rtol)
    n = len(exp_probs)
    i = 0
    while i < n:
        j = i
        while j < n and exp_probs[j] == exp_probs[i]:
            j += 1
        a = sorted(g.tobytes() for g in got_genotypes[i:j].astype(np.int8))
        b = sorted(g.tobytes() for g in exp_genotypes[i:j].astype(np.int8))
        assert a == b, (i, j)
        i = j


def multiallelic_units(rng, U, K, H, n_alleles, R, qual=(5, 30), gap=0.15, window=None):
    """Units of known haplotypes over SNVs of mixed allele counts, as `call-exact` meets them: reads [U, R, M, A] (A =
    max(n_alleles)) encoded by encoding.as_probabilistic -- a called allele gets p, every other allele the position has
    (1 - p) / 3, the alleles it lacks 0, a gap NaN except those ([nan, nan, 0] at a biallelic position of 3 alleles) --
    and haplotypes int8 [U, H, M] with allele < n_alleles[j], distinct within a unit.  Reads come from a genotype of K
    of the unit's haplotypes, with errors at rate 1 - p (another allele of the position) and gaps at rate `gap` or
    outside a read window of `window` = (min, max) positions."""
    from mchap_amd.encoding import as_probabilistic

    na = np.asarray(n_alleles, dtype=int)
    M, A = len(na), int(na.max())
    reads = np.empty((U, R, M, A))
    haps = np.zeros((U, H, M), np.int8)
    for u in range(U):
        if np.prod(na.astype(float)) <= 6 * H + 8:  # (few haplotypes exist: all of them)
            pool = np.stack(np.meshgrid(*[np.arange(n) for n in na], indexing="ij"), axis=-1).reshape(-1, M).astype(np.int8)
        else:
            pool = np.unique(np.stack([rng.integers(0, na) for _ in range(6 * H + 8)]).astype(np.int8), axis=0)
        assert len(pool) >= H, "too few distinct haplotypes for the allele counts"
        rng.shuffle(pool)
        haps[u] = pool[:H]
        truth = haps[u][rng.integers(0, H, size=K)]
        src = truth[rng.integers(0, K, size=R)]
        q = rng.integers(qual[0], qual[1] + 1, size=src.shape)
        p = (1.0 - 0.0024) * (1.0 - 10.0 ** (-q / 10.0))
        other = (src + rng.integers(1, na, size=src.shape)) % na
        calls = np.where(rng.random(src.shape) >= p, other, src).astype(np.int8)
        calls[rng.random(src.shape) < gap] = -1
        if window is not None:
            wlen = rng.integers(min(window[0], M), min(window[1], M) + 1, size=R)
            start = (rng.random(R) * (M - wlen + 1)).astype(int)
            pos = np.arange(M)[None, :]
            calls[(pos < start[:, None]) | (pos >= (start + wlen)[:, None])] = -1
        reads[u] = as_probabilistic(calls, na, p)
    return reads, haps
