"""The definition of find-snvs genotype calls in numpy (include/mchap_hip.h mchap_snv_genotypes_device): the exact
caller's posterior mode restricted to one position, as a closed form over a sample's allele depths.  The tests hold the kernel to
this file, and this file to the oracle (test_find_snvs_genotypes_host.py)."""
import itertools
import math
from functools import lru_cache

import numpy as np


@lru_cache(maxsize=None)
def genotypes(m, K):
    """The multisets of K of m alleles in VCF genotype order: int [G, K], each row ascending."""
    gs = sorted(itertools.combinations_with_replacement(range(m), K), key=lambda g: g[::-1])
    return np.array(gs, dtype=np.int64).reshape(len(gs), K)


@lru_cache(maxsize=None)
def dosages(m, K):
    """int [G, m]: copies of each allele in each genotype of genotypes(m, K)."""
    g = genotypes(m, K)
    return (g[:, :, None] == np.arange(m)).sum(axis=1)


def log_genotype_prior(genotype, m, F, frequencies=None):
    """The reference's calling/prior.py log_genotype_prior(genotype, unique_haplotypes=m, inbreeding=F, frequencies)."""
    K = len(genotype)
    dose = np.bincount(genotype, minlength=m)
    if F == 0:
        ln_perms = math.lgamma(K + 1) - sum(math.lgamma(int(c) + 1) for c in dose)
        if frequencies is None:
            return ln_perms - K * math.log(m)
        return ln_perms + math.log(float(np.prod([frequencies[a] for a in genotype])))
    alphas = (np.full(m, 1.0 / m) if frequencies is None else np.asarray(frequencies, dtype=float)) * ((1 - F) / F)
    total = float(alphas.sum())
    out = math.lgamma(K + 1) + math.lgamma(total) - math.lgamma(K + total)
    for a in range(m):
        if dose[a] > 0:
            out += math.lgamma(dose[a] + alphas[a]) - (math.lgamma(dose[a] + 1) + math.lgamma(alphas[a]))
    return out


@lru_cache(maxsize=4096)
def _prior_terms(m, K, F, frequencies):
    fr = None if frequencies is None else np.array(frequencies)
    return np.array([log_genotype_prior(g, m, F, fr) for g in genotypes(m, K)])


def log_posterior_terms(d, K, error_rate, prior=None):
    """llk(g) + prior(g) for every genotype of ploidy K over the len(d) enumerated alleles with depths d, in VCF order (float64).
    prior: None (flat over the genotypes) or (F, frequencies or None)."""
    d = np.asarray(d, dtype=np.int64)
    m = len(d)
    p_call = 1.0 - error_rate
    p_other = (1.0 - p_call) / 3.0
    C = dosages(m, K)
    with np.errstate(divide="ignore"):
        logt = np.log((np.arange(K + 1) * p_call + (K - np.arange(K + 1)) * p_other) / K)
    lp = np.zeros(len(C))
    for a in range(m):
        if d[a] > 0:  # a term without depth is skipped: error_rate 0 gives -inf only where a seen allele is absent
            lp = lp + float(d[a]) * logt[C[:, a]]
    if prior is not None:
        F, fr = prior
        lp = lp + _prior_terms(m, K, float(F), None if fr is None else tuple(float(x) for x in fr))
    return lp


def mode(d, K, error_rate, prior=None):
    """(index of the mode: the first maximum in VCF order, its posterior probability, the gap between the two highest posterior
    probabilities), or None for a no-call: no depth, a zero prior frequency, or no genotype of non-zero likelihood."""
    d = np.asarray(d, dtype=np.int64)
    if d.sum() == 0:
        return None
    if prior is not None and prior[1] is not None and not (np.asarray(prior[1]) > 0).all():
        return None
    lp = log_posterior_terms(d, K, error_rate, prior)
    mx = lp.max()
    if mx == -np.inf:
        return None
    lse = mx + math.log(np.exp(lp - mx).sum())
    p = np.exp(lp - lse)
    i = int(np.argmax(lp))
    top = np.sort(p)[::-1]
    return i, float(p[i]), float(top[0] - top[1]) if len(top) > 1 else 1.0


def record_flag(order, keep_by_allele):
    """The filter launch's flag of a record: order = the four allele indices in VCF order (reference first), keep by allele index;
    REFMASKED when the reference allele is not kept."""
    f = 1
    for a in range(4):
        f |= int(bool(keep_by_allele[a])) << (1 + a)
    for i, a in enumerate(order):
        f |= int(a) << (8 + 2 * i)
    if not keep_by_allele[order[0]]:
        f |= 1 << 16
    return f


def enumerated_alleles(flag):
    """A filter flag -> (allele indices A C G T = 0..3 of the enumerated alleles in VCF order, REFMASKED)."""
    flag = int(flag)
    masked = bool((flag >> 16) & 1)
    out = []
    for i in range(4):
        a = (flag >> (8 + 2 * i)) & 3
        listed = i == 0 or bool((flag >> (1 + a)) & 1)
        if listed and not (i == 0 and masked):
            out.append(a)
    return out, masked


def call(depth, flags, admf, ploidy, inbreeding=None, frequencies=None, error_rate=0.0024):
    """What find_snvs.genotypes_device computes: -> (gt_index int32 [P, S], gpm float64 [P, S], gap float64 [P, S]); -1 / NaN /
    NaN for a row that is no record and for a no-call."""
    depth = np.asarray(depth)
    P, S = depth.shape[:2]
    ploidy = np.broadcast_to(np.asarray(ploidy, dtype=np.int64), (S,))
    if inbreeding is None:
        inbreeding = 0.0 if frequencies == "ADMF" else np.nan
    F = np.broadcast_to(np.asarray(inbreeding, dtype=np.float64), (S,))
    gt = np.full((P, S), -1, dtype=np.int32)
    gpm = np.full((P, S), np.nan)
    gap = np.full((P, S), np.nan)
    for r in range(P):
        if not int(flags[r]) & 1:
            continue
        alleles, _ = enumerated_alleles(flags[r])
        fr = None
        if frequencies == "ADMF":
            fr = np.asarray(admf[r], dtype=np.float64)[alleles]
            fr = fr / fr.sum()
        for s in range(S):
            prior = None if np.isnan(F[s]) else (float(F[s]), fr)
            got = mode(depth[r, s][alleles], int(ploidy[s]), error_rate, prior)
            if got is not None:
                gt[r, s], gpm[r, s], gap[r, s] = got
    return gt, gpm, gap
