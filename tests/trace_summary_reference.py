"""The definition of the trace summaries (csrc/posterior_kernel.hpp: trace_posterior_kernel, trace_incongruence_kernel) in plain
Python: dicts, tuples, Fractions and floats, nothing of mchap_amd.  tests/test_trace_summary_reference.py anchors it on the host
classes; tests/test_gpu_trace_summary_kernels.py holds the kernels to it.

A state is a tuple of Python ints in ascending order: `ploidy` haplotypes of up to 128 bits each (de novo), or `ploidy` allele
indices (calling).  A trace is one list of states per chain, burn-in already removed."""
from fractions import Fraction

import numpy as np


def support_of(state):
    """The state's distinct haplotypes (alleles) in sorted order."""
    return tuple(sorted(set(state)))


class Summary(object):
    """states / counts: the distinct states by rank and their occurrences; n_obs; labels[r]: the first rank with r's support;
    mode_index, mode_state, mode_count: the first-ranked state of the mode support; support_size: the genotypes of that support;
    spm (the float sum as the definition accumulates it), spm_exact (Fraction), gpm."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def posterior(chains):
    """Distinct states in merged order (chain-major, steps ascending) with counts from a dict, ranked by count descending and then
    first appearance descending (classes.py posterior(), DESIGN "Known reference quirks"); the supports in order of their first
    rank, each sum accumulated in float64 one `count / N` after the other in ranked order; the first maximum of those sums."""
    merged = [s for chain in chains for s in chain]
    n_obs = len(merged)
    counts = {}
    for s in merged:
        counts[s] = counts.get(s, 0) + 1
    distinct = list(counts)  # a dict keeps insertion order: first appearance
    order = sorted(range(len(distinct)), key=lambda e: (-counts[distinct[e]], -e))
    states = [distinct[e] for e in order]
    cnt = [counts[s] for s in states]
    first_rank, sums, exact, size = {}, {}, {}, {}
    labels = []
    for r, s in enumerate(states):
        key = support_of(s)
        if key not in first_rank:
            first_rank[key] = r
            sums[key] = float(cnt[r]) / float(n_obs)
            exact[key] = Fraction(cnt[r], n_obs)
            size[key] = 1
        else:
            sums[key] = sums[key] + float(cnt[r]) / float(n_obs)
            exact[key] += Fraction(cnt[r], n_obs)
            size[key] += 1
        labels.append(first_rank[key])
    best = None
    for key in first_rank:  # order of first rank
        if best is None or sums[key] > sums[best]:
            best = key
    if best is None:
        return Summary(states=[], counts=[], n_obs=0, labels=[], mode_index=-1, mode_state=None, mode_count=0, support=None,
                       support_size=0, spm=float("nan"), spm_exact=None, gpm=float("nan"))
    m = first_rank[best]
    return Summary(states=states, counts=cnt, n_obs=n_obs, labels=labels, mode_index=m, mode_state=states[m], mode_count=cnt[m],
                   support=best, support_size=size[best], spm=sums[best], spm_exact=exact[best], gpm=float(cnt[m]) / float(n_obs))


def overflowed_table(chains, cap):
    """What a table of `cap` states keeps of a trace with more distinct states: the first `cap` in merged order, each with all its
    occurrences, ranked among themselves by the same rule.  (states, counts)"""
    counts = {}
    for chain in chains:
        for s in chain:
            counts[s] = counts.get(s, 0) + 1
    kept = list(counts)[:cap]
    order = sorted(range(len(kept)), key=lambda e: (-counts[kept[e]], -e))
    return [kept[e] for e in order], [counts[kept[e]] for e in order]


def spm_bound(t):
    """What a float64 sum of t terms count / N may differ from the exact one by: each term one rounding of a value at most 1, each
    of the t - 1 additions one rounding of a partial sum at most 1 -- under 2 t half-ulps of 1."""
    return 2 * t * 2.0 ** -53


def incongruence_denovo(chains, threshold):
    """GenotypeMultiTrace.replicate_incongruence: per chain the mode support, kept if its float sum reaches the threshold."""
    kept = []
    for chain in chains:
        p = posterior([chain])
        if p.n_obs and p.spm >= threshold:
            kept.append(p.support)
    if len(set(kept)) <= 1:
        return 0
    return 2 if len(set().union(*kept)) > len(kept[0]) else 1


def incongruence_calling(chains, threshold):
    """calling_mcmc.py replicate_incongruence: the kept chains are compared by mode genotype, copies kept."""
    kept = []
    for chain in chains:
        p = posterior([chain])
        if p.n_obs and p.spm >= threshold:
            kept.append(p.mode_state)
    if len(set(kept)) <= 1:
        return 0
    named = set()
    for g in kept:
        named |= set(g)
    return 2 if len(named) > len(kept[0]) else 1


def distinct_count(chains):
    return len({s for chain in chains for s in chain})


# ---- the uint64 layouts of include/mchap_hip.h ----
MASK64 = (1 << 64) - 1


def pack_state(state, wph):
    """A de novo state as its words: one per haplotype, or two with the most significant first; haplotypes ascending as 128-bit
    values (which the tuple already is)."""
    assert list(state) == sorted(state)
    if wph == 1:
        assert all(0 <= h <= MASK64 for h in state)
        return [int(h) for h in state]
    assert wph == 2 and all(0 <= h < (1 << 128) for h in state)
    out = []
    for h in state:
        out += [int(h) >> 64, int(h) & MASK64]
    return out


def pack_trace(chains, wph):
    """[chains][steps] states -> uint64 [chains, steps, ploidy * wph]."""
    return np.array([[pack_state(s, wph) for s in chain] for chain in chains], dtype=np.uint64)


def pack_alleles(chains):
    """[chains][steps] calling states -> int64 [chains, steps, ploidy], alleles ascending."""
    for chain in chains:
        for s in chain:
            assert list(s) == sorted(s)
    return np.array([[list(s) for s in chain] for chain in chains], dtype=np.int64)


def unpack_haplotypes(chains, n_bits):
    """[chains][steps] de novo states -> int8 [chains, steps, ploidy, n_bits], bit n_bits - 1 first: the biallelic genotypes whose
    canonical (lexicographic) order is the states' ascending order."""
    out = np.zeros((len(chains), len(chains[0]), len(chains[0][0]), n_bits), dtype=np.int8)
    rows = {}
    for c, chain in enumerate(chains):
        for s, state in enumerate(chain):
            for k, h in enumerate(state):
                if h not in rows:
                    assert 0 <= h < (1 << n_bits)
                    rows[h] = np.array([(h >> (n_bits - 1 - j)) & 1 for j in range(n_bits)], dtype=np.int8)
                out[c, s, k] = rows[h]
    return out
