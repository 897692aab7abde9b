"""One iteration of the prior allele-frequency estimate in long double, for the tests of the estimate's kernels
(tests/test_estimate_reference.py, tests/test_gpu_estimate_kernels.py, tests/fuzz_estimate.py): plain numpy, the genotype table
built from itertools, and the log prior written as sums of logarithms -- no lgamma anywhere, so that the reference does not share
the rounding of the kernels' `lgamma(d + alpha) - lgamma(d + 1) - lgamma(alpha)`.  A float64 restatement of the kernels' own form
(math.lgamma) stands beside it: what separates the two is the loss of the formula, not of an implementation."""
import functools
import itertools
import math

import numpy as np

LD = np.longdouble
# the reference has to carry more digits than the float64 it judges: a 64-bit significand (x87 extended precision)
assert np.finfo(LD).eps < 2e-19, "np.longdouble is no wider than float64 on this host: %r" % np.finfo(LD).eps


@functools.lru_cache(maxsize=64)
def genotype_table(H, K):
    """int64 [G, K]: the ascending multisets of K alleles out of H in VCF order (the highest allele most significant)."""
    G = math.comb(H + K - 1, K)
    g = np.fromiter(itertools.chain.from_iterable(itertools.combinations_with_replacement(range(H), K)), dtype=np.int64,
                    count=G * K).reshape(G, K)
    g = g[np.lexsort(tuple(g[:, k] for k in range(K)))]   # (lexsort: the last key is the primary one)
    g.setflags(write=False)
    return g


def _occurrence(g):
    """[G, K]: how many copies of allele g[i, k] stand before position k in genotype i (the alleles are ascending)."""
    occ = np.zeros(g.shape, dtype=np.int64)
    for k in range(1, g.shape[1]):
        occ[:, k] = np.where(g[:, k] == g[:, k - 1], occ[:, k - 1] + 1, 0)
    return occ


def log_prior(g, H, K, F, f):
    """longdouble [G]: the log prior of every genotype up to a constant.  F > 0 (Dirichlet-multinomial, alpha = f (1 - F) / F):
    sum_h sum_{i < d_h} (log(alpha_h + i) - log(i + 1)); F = 0 (multinomial): sum_h (d_h log f_h - log d_h!).  Both are a sum over
    the K positions of a term of (allele, copies of it before): a [H, K] table, gathered.  An allele of frequency 0 that occurs
    gives log(0) = -inf at its first copy; one that does not occur is never looked up."""
    f = np.asarray(f, dtype=np.float64).astype(LD)
    i = np.arange(K).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        if F > 0:
            alpha = f * ((LD(1) - LD(F)) / LD(F))
            term = np.log(alpha[:, None] + i[None, :]) - np.log(i + 1)[None, :]
        else:
            term = np.log(f)[:, None] - np.log(i + 1)[None, :]
        occ = _occurrence(g)
        lp = np.zeros(len(g), dtype=LD)
        for k in range(K):
            lp += term[g[:, k], occ[:, k]]
    return lp


def unit_allele_counts(llk, g, H, K, F, f):
    """longdouble [H]: K * freqs_s, the expected allele counts of one unit with log likelihoods llk [G] under prior (F, f).  All
    NaN where no genotype has a finite llk + log prior (0 / 0, as the definition's posterior) or where f holds a NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        lj = np.asarray(llk, dtype=np.float64).astype(LD) + log_prior(g, H, K, F, f)
        m = np.max(lj)
        if not np.isfinite(m):
            return np.full(H, np.nan, dtype=LD)
        p = np.exp(lj - m)
    counts = np.zeros(H, dtype=LD)
    for k in range(K):
        np.add.at(counts, g[:, k], p)
    return counts / np.sum(p)


def iterate(records):
    """records: [dict(H, f float64 [H], units [(llk float64 [G], K, F)])] -> [f' float64 [H]] with f' = sum_s counts_s / sum_s K_s
    in long double, rounded to float64 at the end."""
    out = []
    for r in records:
        H = int(r["H"])
        acc = np.zeros(H, dtype=LD)
        ktot = 0
        for llk, K, F in r["units"]:
            acc += unit_allele_counts(llk, genotype_table(H, int(K)), H, int(K), float(F), r["f"])
            ktot += int(K)
        out.append((acc / LD(ktot)).astype(np.float64))
    return out


# ---- the kernels' own form in float64 (exact_em_counts_kernel, calling_log_prior): the envelope of F is measured with it ----
def _lgamma(x):
    return math.inf if x == 0.0 else math.lgamma(x)


def unit_allele_counts_lgamma(llk, g, H, K, F, f):
    """float64 [H]: the same quantity the way the kernels form it -- the table lgd[h][d] = lgamma(d + alpha_h) - (lgamma(d + 1) +
    lgamma(alpha_h)) and the constant lgamma(K + 1) + lgamma(sum alpha) - lgamma(K + sum alpha) for F > 0; lgamma(K + 1) - sum
    lgamma(d_h + 1) + log(prod f) for F = 0 -- with math.lgamma."""
    f = np.asarray(f, dtype=np.float64)
    occ = _occurrence(g)
    last = np.ones(g.shape, dtype=bool)   # the last copy of its allele: the run length is occ + 1 there
    last[:, :-1] = g[:, 1:] != g[:, :-1]
    lgf = np.array([math.lgamma(d + 1.0) for d in range(K + 1)])
    with np.errstate(divide="ignore", invalid="ignore"):
        if F > 0:
            scale = (1.0 - F) / F
            alpha = f * scale
            lgd = np.array([[0.0 if d == 0 else _lgamma(d + a) - (math.lgamma(d + 1.0) + _lgamma(a)) for d in range(K + 1)] for a in alpha])
            sa = 0.0
            for a in alpha:
                sa += a
            left = (math.lgamma(K + 1.0) + math.lgamma(sa)) - math.lgamma(K + sa)
            prod = np.zeros(len(g))
            for k in range(K):
                prod += np.where(last[:, k], lgd[g[:, k], occ[:, k] + 1], 0.0)
            lp = left + prod
        else:
            den = np.zeros(len(g))
            prod = np.ones(len(g))
            for k in range(K):
                den += np.where(last[:, k], lgf[occ[:, k] + 1], 0.0)
                prod *= f[g[:, k]]
            lp = (lgf[K] - den) + np.log(prod)
        lj = np.asarray(llk, dtype=np.float64) + lp
        m = np.max(lj)
        if not np.isfinite(m):
            return np.full(H, np.nan)
        p = np.where(lj > -np.inf, np.exp(lj - m), 0.0)
    counts = np.zeros(H)
    for k in range(K):
        counts += np.bincount(g[:, k], weights=p, minlength=H)
    return counts / p.sum()


def iterate_lgamma(records):
    """iterate() on unit_allele_counts_lgamma, in float64 throughout."""
    out = []
    for r in records:
        H = int(r["H"])
        acc = np.zeros(H)
        ktot = 0
        for llk, K, F in r["units"]:
            acc += unit_allele_counts_lgamma(llk, genotype_table(H, int(K)), H, int(K), float(F), r["f"])
            ktot += int(K)
        out.append(acc / float(ktot))
    return out


def deviation(got, want, rel, floor):
    """(every element within rel * |want| + floor, the largest |got - want| / max(|want|, floor / rel)): NaN anywhere fails."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    ok = bool(np.all(err <= rel * np.abs(want) + floor))
    return ok, float(np.max(err / np.maximum(np.abs(want), floor / rel))) if err.size else 0.0
