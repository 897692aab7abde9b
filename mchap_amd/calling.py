"""Exact genotype caller on MI355X HIP kernels: drop-in for the module-level functions of the reference's
mchap/calling/exact.py (posterior_mode 156-249, genotype_likelihoods 266-292, genotype_posteriors 295-329,
posterior_allele_frequencies 332-369, alternate_dosage_posteriors 372-407) -- same names, arguments and results.
`posterior_mode_batch` runs many units that share a shape in one launch.  No CPU fallback.
"""
import ctypes as C
from itertools import combinations_with_replacement
from math import comb

import numpy as np

from . import _lib

__all__ = [
    "posterior_mode",
    "posterior_mode_batch",
    "allele_read_support",
    "cross_genotype_prior",
    "cross_genotype_posteriors",
    "family_genotype_posteriors",
    "genotype_likelihoods",
    "genotype_posteriors",
    "posterior_allele_frequencies",
    "alternate_dosage_posteriors",
    "count_unique_genotypes",
    "genotypes_in_vcf_order",
    "call_arrays_batch",
    "genotype_alleles_as_index",
    "index_as_genotype_alleles",
]


def count_unique_genotypes(u_haps, ploidy):
    """Number of genotypes of `ploidy` over `u_haps` haplotypes (reference combinatorics.py:35-54)."""
    return comb(u_haps + ploidy - 1, ploidy) if u_haps > 0 else 0


def _cwr(n, k):
    return comb(n + k - 1, k) if n > 0 else 0


def genotype_alleles_as_index(alleles):
    """VCF order index of ascending alleles (reference jitutils.py:253-276)."""
    index = 0
    for i, a in enumerate(alleles):
        if a < 0:
            raise ValueError("Allele numbers must be >= 0.")
        index += _cwr(int(a), i + 1)
    return index


def index_as_genotype_alleles(index, ploidy):
    """Alleles of the genotype at a VCF order index (reference jitutils.py:279-318)."""
    out = np.full(ploidy, -2, np.int64)
    if index < 0:
        out[:] = -1
        return out
    remainder = index
    for p in range(ploidy, 0, -1):
        n, new, prev = -1, 0, 0
        while new <= remainder:
            n += 1
            prev = new
            new = _cwr(n, p)
        remainder -= prev
        out[p - 1] = n - 1
    return out


def _reads(reads, read_counts):
    reads = np.ascontiguousarray(reads, dtype=np.float64)
    n_reads = reads.shape[0]
    if n_reads == 0:
        # a missing sample is one all-NaN read (reference assemble/mcmc.py:132-137, snpcalling.py:42-46)
        reads = np.full((1,) + reads.shape[1:], np.nan)
        read_counts = None
    rc = None if read_counts is None else np.ascontiguousarray(read_counts, dtype=np.int64)
    return reads, rc


def genotype_likelihoods(reads, ploidy, haplotypes, read_counts=None):
    """Log likelihood of every genotype in VCF order, float32 as the reference stores it."""
    reads, rc = _reads(reads, read_counts)
    haps = np.ascontiguousarray(haplotypes, dtype=np.int8)
    R, M, A = reads.shape
    G = count_unique_genotypes(len(haps), ploidy)
    out = np.full(G, np.nan, np.float32)
    _lib.check(_lib.lib().mchap_exact_genotype_likelihoods(
        _lib.ptr(reads), R, M, A, _lib.ptr(rc), _lib.ptr(haps), len(haps), int(ploidy), _lib.ptr(out), None))
    return out


def genotype_posteriors(log_likelihoods, ploidy, n_alleles, prior=None):
    """Posterior probability of every genotype in VCF order (float64 array; float32 arithmetic when the
    likelihoods are float32, as in the reference)."""
    llks = np.ascontiguousarray(log_likelihoods)
    if llks.dtype not in (np.float32, np.float64):
        llks = llks.astype(np.float64)
    has = 0 if prior is None else 1
    F = 0.0 if prior is None else float(prior[0])
    fr = None if (prior is None or prior[1] is None) else np.ascontiguousarray(prior[1], dtype=np.float64)
    out = np.zeros(len(llks), dtype=np.float64)
    _lib.check(_lib.lib().mchap_exact_genotype_posteriors(
        _lib.ptr(llks), int(llks.dtype == np.float32), C.c_int64(len(llks)), int(ploidy), int(n_alleles), has,
        C.c_double(F), _lib.ptr(fr), _lib.ptr(out)))
    return out


def posterior_allele_frequencies(posteriors, ploidy, n_alleles):
    """(mean allele frequencies, allele counts, occurrence probabilities) of a posterior over VCF ordered genotypes
    (one pass of the device kernel over the array)."""
    post = np.ascontiguousarray(posteriors, dtype=np.float64)
    freqs, counts, occur = np.zeros(n_alleles), np.zeros(n_alleles), np.zeros(n_alleles)
    _lib.check(_lib.lib().mchap_exact_posterior_summaries(
        _lib.ptr(post), C.c_int64(len(post)), int(ploidy), int(n_alleles), None, None, None, _lib.ptr(freqs), _lib.ptr(counts),
        _lib.ptr(occur)))
    return freqs, counts, occur


def genotypes_in_vcf_order(n, ploidy):
    """Alleles [n, ploidy] of the first n genotypes in VCF order: the combinatorial number system read from the
    highest position down (what index_as_genotype_alleles does one index at a time), vectorised over the indices."""
    rem = np.arange(n, dtype=np.int64)
    out = np.zeros((n, ploidy), dtype=np.int64)
    top = 1
    while _cwr(top, ploidy) <= max(n - 1, 0):
        top += 1
    for p in range(ploidy, 0, -1):
        table = np.array([_cwr(a, p) for a in range(top + 2)], dtype=np.int64)  # genotypes of p alleles below allele a
        a = np.searchsorted(table, rem, side="right") - 1
        out[:, p - 1] = a
        rem = rem - table[a]
    return out


def alternate_dosage_posteriors(genotype_alleles, probabilities):
    """Posterior of every dosage variant of the genotype's support (calling/exact.py:363-407): the genotypes that hold each allele
    of the support at least once, in VCF order, with their entries of `probabilities`.  A variant is the support plus a multiset of
    `ploidy - len(support)` extra copies; all of them are formed as one array (multisets as rows of indices into the support), their
    VCF indices by the combinatorial number system over the sorted rows, and the rows ordered by index."""
    support = np.unique(np.asarray(genotype_alleles))
    ploidy, extra = len(genotype_alleles), len(genotype_alleles) - len(support)
    combos = list(combinations_with_replacement(range(len(support)), extra))  # (extra == 0: the one empty multiset)
    picks = np.array(combos, dtype=np.int64).reshape(len(combos), extra)
    rows = np.sort(np.concatenate([np.broadcast_to(support, (len(picks), len(support))), support[picks]], axis=1), axis=1).astype(np.int64)
    # index of a sorted row a_1 <= ... <= a_K in VCF order: sum_k C(a_k + k - 1, k)
    index = np.zeros(len(rows), dtype=np.int64)
    for k in range(1, ploidy + 1):
        index += np.array([comb(int(a) + k - 1, k) for a in rows[:, k - 1]], dtype=np.int64)
    order = np.argsort(index, kind="stable")
    return rows[order], np.asarray(probabilities, dtype=float)[index[order]]


def posterior_mode_batch(reads, ploidy, haplotypes, read_counts=None, prior=None, return_support_prob=False,
                         return_posterior_frequencies=False, return_posterior_occurrence=False):
    """posterior_mode for a batch: reads [U, R, M, A], haplotypes [U, H, M] (or [H, M] shared),
    read_counts [U, R] or None, prior = None | (inbreeding scalar or [U], frequencies None | [H] | [U, H])."""
    reads = np.ascontiguousarray(reads, dtype=np.float64)
    U, R, M, A = reads.shape
    haps = np.asarray(haplotypes, dtype=np.int8)
    if haps.ndim == 2:
        haps = np.broadcast_to(haps, (U,) + haps.shape)
    haps = np.ascontiguousarray(haps)
    H = haps.shape[1]
    rc = None if read_counts is None else np.ascontiguousarray(read_counts, dtype=np.int64)
    has = 0 if prior is None else 1
    F = fr = None
    if prior is not None:
        F = np.ascontiguousarray(np.broadcast_to(np.asarray(prior[0], dtype=np.float64), (U,)))
        if prior[1] is not None:
            fr = np.ascontiguousarray(np.broadcast_to(np.asarray(prior[1], dtype=np.float64), (U, H)))
    K = int(ploidy)
    alleles = np.zeros((U, K), np.int64)
    mllk, mprob = np.zeros(U), np.zeros(U)
    sprob = np.zeros(U) if return_support_prob else None
    want_f = return_posterior_frequencies or return_posterior_occurrence
    freqs = np.zeros((U, H)) if want_f else None
    occur = np.zeros((U, H)) if want_f else None
    _lib.check(_lib.lib().mchap_exact_posterior_mode_batch(
        U, _lib.ptr(reads), R, M, A, _lib.ptr(rc), _lib.ptr(haps), H, K, has, _lib.ptr(F), _lib.ptr(fr),
        _lib.ptr(alleles), _lib.ptr(mllk), _lib.ptr(mprob), _lib.ptr(sprob), _lib.ptr(freqs), _lib.ptr(occur)))
    result = [alleles, mllk, mprob]
    if return_support_prob:
        result.append(sprob)
    if return_posterior_frequencies:
        result.append(freqs)
    if return_posterior_occurrence:
        result.append(occur)
    return tuple(result)


def posterior_mode(reads, ploidy, haplotypes, read_counts=None, prior=None, return_support_prob=False,
                   return_posterior_frequencies=False, return_posterior_occurrence=False):
    """Posterior mode genotype with statistics from a set of known haplotypes (streaming form: no array over
    all genotypes is returned).  Returns (mode_alleles, mode_llk, mode_probability[, mode_support_probability]
    [, mean_allele_frequencies][, allele_occurrence_probability])."""
    reads, rc = _reads(reads, read_counts)
    out = posterior_mode_batch(reads[None], ploidy, np.asarray(haplotypes)[None], None if rc is None else rc[None], prior,
                               return_support_prob, return_posterior_frequencies, return_posterior_occurrence)
    res = [out[0][0], float(out[1][0]), float(out[2][0])]
    k = 3
    if return_support_prob:
        res.append(float(out[k][0]))
        k += 1
    if return_posterior_frequencies:
        res.append(out[k][0])
        k += 1
    if return_posterior_occurrence:
        res.append(out[k][0])
    return tuple(res)


def allele_read_support(reads, ploidy, haplotypes, read_counts=None, prior=None, per_read=False):
    """Expected read depth of every haplotype of one unit (not a reference function; the definition: application.allele_support_unit):
    depth float64 [H], the responsibility of haplotype h for every read under every genotype, averaged over the genotype posterior
    and summed over the reads with their weights -- sum(depth) is the unit's read weight.  reads [R, M, A], haplotypes [H, M],
    read_counts [R] or None, prior = None (the flat genotype prior) | (inbreeding, frequencies None | [H]).  per_read=True:
    (depth, read_post float64 [R, H]), every row of a read with weight summing to 1.  NaN where no genotype is finite."""
    import torch

    from .device import ExactDeviceBatch, ExactReadSupport

    haps = np.ascontiguousarray(haplotypes, dtype=np.int8)
    if len(reads) == 0:   # (no reads: nothing to assign)
        return (np.zeros(len(haps)), np.zeros((0, len(haps)))) if per_read else np.zeros(len(haps))
    reads, rc = _reads(reads, read_counts)
    batch = ExactDeviceBatch(reads[None], int(ploidy), haps[None], None if rc is None else rc[None], None, cache_joint=False)
    F = fr = None
    if prior is not None:
        F = [float(prior[0])]
        fr = np.full((1, len(haps)), 1.0 / len(haps)) if prior[1] is None else np.asarray(prior[1], dtype=np.float64).reshape(1, -1)
    got = ExactReadSupport(batch.device).add_group(batch, batch.run_llks64(), F, [0], fr, per_read=per_read)
    torch.cuda.synchronize()
    if per_read:
        return got[0].cpu().numpy()[0], got[1].cpu().numpy()[0]
    return got.cpu().numpy()[0]


def cross_genotype_prior(parent_posteriors_p, ploidy_p, parent_posteriors_q, ploidy_q, n_alleles, gamete_error=(0, 0), frequencies=None):
    """The distribution X float64 [G_c] of the cross of two parents over the genotypes of ploidy ploidy_p / 2 + ploidy_q / 2 (not
    a reference function; the definition: application.cross_prior_tables): parent_posteriors_p / _q the parents' genotype
    posteriors [G_p] / [G_q] in VCF order, even ploidies, n_alleles haplotypes; gamete_error (e_p, e_q) mixes the multinomial of
    `frequencies` [n_alleles] (None: flat) into either gamete table.  No double reduction; the parents are independent."""
    import torch

    from .device import ExactCross

    H = int(n_alleles)
    fr = np.full((1, H), 1.0 / H) if frequencies is None else np.asarray(frequencies, dtype=np.float64).reshape(1, H)
    dev = ExactCross()
    gam = []
    for p, K, e in ((parent_posteriors_p, ploidy_p, gamete_error[0]), (parent_posteriors_q, ploidy_q, gamete_error[1])):
        with np.errstate(divide="ignore"):
            # (the posterior itself as the likelihood under the flat genotype prior: the kernel's p is the given one again)
            llk = torch.from_numpy(np.log(np.ascontiguousarray(p, dtype=np.float64))).to(dev.device)
        gam.append(dev.gametes(llk, H, int(K), None, [0], fr, [float(e)]))
    log_x = dev.cross_prior(gam[0], gam[1], H, int(ploidy_p), int(ploidy_q))
    return torch.exp(log_x)[0].cpu().numpy()


def selfing_genotype_prior(parent_posteriors, ploidy, n_alleles, gamete_error=0, frequencies=None):
    """The distribution S float64 [G] of the progeny of a SELFED parent over the genotypes of its own ploidy (not a reference
    function; the definition: application.selfing_prior): parent_posteriors the parent's genotype posterior [G] in VCF order -- or
    [n, G] for n parents of one record, and then [n, G] comes back --, an even ploidy, n_alleles haplotypes; gamete_error mixes the
    multinomial of `frequencies` [n_alleles] (None: flat) into each of the two gametes.  The two gametes come from ONE genotype: unless
    the posterior is one-hot this is not cross_genotype_prior of the parent with itself.  Its logarithm feeds
    cross_genotype_posteriors unchanged.  A posterior with a NaN gives NaN throughout, as the definition does.  No double reduction."""
    import torch

    from .device import ExactSelfing

    H = int(n_alleles)
    fr = np.full((1, H), 1.0 / H) if frequencies is None else np.asarray(frequencies, dtype=np.float64).reshape(1, H)
    post = np.ascontiguousarray(parent_posteriors, dtype=np.float64)
    one = post.ndim == 1
    post = np.atleast_2d(post)
    dev = ExactSelfing()
    with np.errstate(divide="ignore"):
        # (the posterior itself as the likelihood under the flat genotype prior: the kernel's p is the given one again)
        llk = torch.from_numpy(np.log(post)).to(dev.device).reshape(-1)
    S = dev.selfing_prior(llk, H, int(ploidy), None, [0] * len(post), fr, float(gamete_error))[1].cpu().numpy()
    S[np.any(np.isnan(post), axis=1)] = np.nan   # (the kernel counts a NaN likelihood as 0: the definition gives NaN throughout)
    return S[0] if one else S


def cross_genotype_posteriors(llks, log_cross_prior):
    """The posterior float64 [G_c] of a progeny with log likelihoods llks [G_c] under the log cross prior [G_c]
    (log of cross_genotype_prior): exp(llks + log_cross_prior - log Z).  NaN where no genotype has a finite term."""
    import torch

    from .device import ExactCross

    dev = ExactCross()
    llk = torch.from_numpy(np.ascontiguousarray(llks, dtype=np.float64)).to(dev.device)
    lx = torch.from_numpy(np.ascontiguousarray(log_cross_prior, dtype=np.float64).reshape(1, -1)).to(dev.device)
    G = int(llk.numel())
    # (the shape is given by the arrays alone: any (H, K) with C(H + K - 1, K) = G streams them alike -- K = 1 over G alleles)
    return dev.posteriors(llk, G, 1, lx, [0], full=True)[4][0].cpu().numpy()


def parentage_log_evidence(gametes_a, gametes_b, llks, n_alleles, t_a, t_b):
    """The cross evidence of progeny under every pair of rows of two gamete tables (not a reference function; the definition:
    application.parentage_unit): gametes_a [n_a, C(H + t_a - 1, t_a)] and gametes_b [n_b, C(H + t_b - 1, t_b)] distributions over the
    gametes of t_a and t_b haplotypes out of n_alleles (VCF order), llks [n, G_c] -- or [G_c] for one progeny -- the log likelihoods
    of progeny of ploidy t_a + t_b.  Returns float64 [n, n_a, n_b] (or [n_a, n_b]):
        log sum_a gametes_a[i][a] sum_b gametes_b[j][b] exp(llks[c][rank(a + b)])."""
    import torch

    from .device import ExactParentage

    dev = ExactParentage()
    llk = np.ascontiguousarray(llks, dtype=np.float64)
    one = llk.ndim == 1
    tables = [torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(g, dtype=np.float64)))[None]).to(dev.device)
              for g in (gametes_a, gametes_b)]
    got = dev.log_evidence(tables[0], tables[1], torch.from_numpy(llk.reshape(-1)).to(dev.device), int(n_alleles), int(t_a), int(t_b))
    out = got.cpu().numpy()[0]
    return out[0] if one else out


def identity_log_bayes_factors(llks, log_prior=None, error=0.01):
    """The identity evidence of every pair of samples at one record (not a reference function; the definition:
    application.identity_unit): llks [n, G] the log likelihoods of n samples of one ploidy, log_prior [G] their normalised log
    genotype prior (None: the flat prior), error in [0, 1].  Returns float64 [n, n], the diagonal NaN:
        log((1 - error) sum_g post_i(g) post_j(g) / prior(g) + error)."""
    import torch
    from math import log

    from .device import ExactIdentity, ExactModelEvidence

    dev = ExactIdentity()
    llk = np.atleast_2d(np.ascontiguousarray(llks, dtype=np.float64))
    n, G = llk.shape
    for_norm = for_a = llk
    if log_prior is not None:
        # (the given prior on top of the flat one the kernels add: its constant comes off again, half of it for the rows a)
        lp = np.asarray(log_prior, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            for_norm, for_a = llk + (lp + log(G)), llk + 0.5 * (lp + log(G))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev.device)  # noqa: E731
    # (the shape is given by the arrays alone: any (H, K) with C(H + K - 1, K) = G streams them alike -- K = 1 over G alleles)
    norm = ExactModelEvidence(dev.device).add_group(up(for_norm).reshape(-1), G, 1, None, None, None).reshape(1, n).contiguous()
    return dev.log_bayes_factors(up(for_a).reshape(-1), G, 1, None, None, None, norm, error).cpu().numpy()[0]


def family_genotype_posteriors(llks_p, ploidy_p, llks_q, ploidy_q, llks_progeny, n_alleles, log_prior_p=None, log_prior_q=None,
                               gamete_error=(0, 0), frequencies=None):
    """The joint call of one nuclear family (not a reference function; the definition: application.family_unit): parents with log
    likelihoods llks_p [G_p], llks_q [G_q] (VCF order, even ploidies, n_alleles haplotypes) and log genotype priors log_prior_p /
    _q [G] (None: the flat genotype prior), progeny with log likelihoods llks_progeny[c] [G_c] of ploidy ploidy_p / 2 +
    ploidy_q / 2 (None for a progeny without reads: it informs nothing and is called from the rest of the family);
    gamete_error (e_p, e_q) mixes the multinomial of `frequencies` [n_alleles] (None: flat) into the gametes.  Returns
    (post_p [G_p], post_q [G_q], [q_c [G_c]], log_z, pred [n]): the parents' and the progeny's marginals in the exact joint
    posterior, the log evidence of the family, and every progeny's predictive log evidence given the rest of the family.  All NaN
    where the joint has no mass: a sample without a finite genotype, or parents that cannot have a progeny at a gamete error of 0."""
    import torch
    from math import log

    from .device import ExactFamily

    H = int(n_alleles)
    fr = np.full((1, H), 1.0 / H) if frequencies is None else np.asarray(frequencies, dtype=np.float64).reshape(1, H)
    dev = ExactFamily()
    tables, shift = [], 0.0
    for llk, lp in ((llks_p, log_prior_p), (llks_q, log_prior_q)):
        llk = np.ascontiguousarray(llk, dtype=np.float64)
        if lp is not None:
            # (the given prior on top of the flat one the kernel adds: its constant comes off the evidence again)
            llk = llk + np.asarray(lp, dtype=np.float64)
            shift += log(len(llk))
        tables.append(torch.from_numpy(llk).to(dev.device))
    n = len(llks_progeny)
    reads = np.array([[0 if x is None else 1 for x in llks_progeny]], dtype=np.int32).reshape(1, n)
    GC = ExactFamily._shape(H, int(ploidy_p) // 2 + int(ploidy_q) // 2)
    progeny = None
    if n:
        progeny = torch.from_numpy(np.concatenate([np.zeros(GC) if x is None else np.ascontiguousarray(x, dtype=np.float64)
                                                   for x in llks_progeny])).to(dev.device)
    got = dev.call(tables[0], tables[1], progeny, H, int(ploidy_p), int(ploidy_q), fr, gamete_error, progeny_reads=reads, full=True)
    q = got["q"].cpu().numpy()[0]
    return (got["post_p"].cpu().numpy()[0], got["post_q"].cpu().numpy()[0], [q[c] for c in range(n)],
            float(got["log_z"].cpu().numpy()[0]) + shift, got["pred"].cpu().numpy()[0])


def call_arrays_batch(reads, ploidy, haplotypes, read_counts=None, prior=None, return_arrays=True):
    """The array form of the exact caller for a batch (what `mchap call-exact --report GL GP` computes per sample,
    reference application/call_exact.py:126-159): genotype_likelihoods (float32) -> genotype_posteriors -> the
    posterior array's mode, the probability of the mode's support, posterior_allele_frequencies -- one device call,
    no host loop over genotypes or units.

    reads [U, R, M, A], haplotypes [U, H, M] or [H, M], read_counts [U, R] or None,
    prior = None | (inbreeding scalar or [U], frequencies None | [H] | [U, H]).
    Returns a dict: alleles [U, K], prob [U], support_prob [U], freqs / counts / occur [U, H] and, with
    return_arrays, llks float32 [U, G] and posteriors float64 [U, G]."""
    from .device import ExactDeviceBatch

    batch = ExactDeviceBatch(reads, ploidy, haplotypes, read_counts, prior)
    batch.run(arrays=True, streaming=False)
    return batch.array_results(return_arrays)
