#!/usr/bin/env python3
"""Generate tests/golden/cross_prior.npz: what the reference gives for the distribution of a cross, as arrays in VCF order.
Part 1 (mchap/assemble/inheritence.py gamete_probabilities, cross_probabilities): drawn parent posteriors for the crosses 2x2, 4x4
and 6x6 over 2, 3 and 4 haplotypes -> the two gamete tables and the cross.  Part 2 (mchap/pedigree/prior.py trio_log_pmf with
lambda = 0): exp of the log pmf of every progeny genotype for one-hot parents at 4x2, 6x4 and 8x8 over 3 haplotypes, gamete errors
(0, 0), (0.01, 0.01) and (0.01, 0.2), a drawn frequency row and one with a zero.  The reference is imported under the identity
shims of tests/golden/_shim.  Build container only (needs /root/reference); the output is data, not source.
Usage: python tests/golden/make_cross_prior.py"""
import itertools
import os
import sys
from math import comb

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")

from mchap.assemble.inheritence import cross_probabilities, gamete_probabilities  # noqa: E402
from mchap.pedigree.prior import trio_log_pmf  # noqa: E402


def table(H, K):
    """The ascending multisets of K out of H in VCF order."""
    return sorted(itertools.combinations_with_replacement(range(H), K), key=lambda t: t[::-1])


def in_vcf_order(multisets, probs, H, K):
    """The reference's (multisets [n, K, 1], probabilities [n]) as an array over table(H, K); what it does not list is 0."""
    index = {t: i for i, t in enumerate(table(H, K))}
    out = np.zeros(len(index))
    for g, p in zip(multisets, probs):
        out[index[tuple(sorted(int(x) for x in g[:, 0]))]] += p
    return out


rng = np.random.default_rng(20261021)
out = {}
names = []
for K in (2, 4, 6):
    for H in (2, 3, 4):
        G = table(H, K)
        pp, pq = rng.dirichlet(np.ones(len(G))), rng.dirichlet(np.ones(len(G)))
        if H == 3:   # (one case with genotypes of probability 0)
            pp[rng.random(len(G)) < 0.5] = 0.0
            pp[0] += 1e-3
            pp /= pp.sum()
        gen = np.array(G, dtype=np.int8)[:, :, None]
        mg, mp = gamete_probabilities(gen, pp)
        qg, qp = gamete_probabilities(gen, pq)
        cg, cp = cross_probabilities(mg, mp, qg, qp)
        name = "part1_%dx%d_H%d" % (K, K, H)
        names.append(name)
        out[name + "_shape"] = np.array([H, K, K])
        out[name + "_pp"], out[name + "_pq"] = pp, pq
        out[name + "_gam_p"] = in_vcf_order(mg, mp, H, K // 2)
        out[name + "_gam_q"] = in_vcf_order(qg, qp, H, K // 2)
        out[name + "_x"] = in_vcf_order(cg, cp, H, K)

H = 3
freqs = np.stack([rng.dirichlet(np.full(H, 2.0)), np.array([0.6, 0.0, 0.4])])
out["part2_freqs"] = freqs
for KP, KQ in ((4, 2), (6, 4), (8, 8)):
    GP, GQ = table(H, KP), table(H, KQ)
    KC = KP // 2 + KQ // 2
    GC = table(H, KC)
    n = max(KP, KQ, KC)
    pad = lambda t: np.array(list(t) + [-1] * (n - len(t)), dtype=np.int64)  # noqa: E731
    picks = [(int(rng.integers(len(GP))), int(rng.integers(len(GQ)))) for _ in range(3)]
    for fi in range(len(freqs)):
        for ep, eq in ((0.0, 0.0), (0.01, 0.01), (0.01, 0.2)):
            for ip, iq in picks:
                x = np.zeros(len(GC))
                with np.errstate(divide="ignore"):
                    logf = np.log(freqs[fi])
                for j, gc in enumerate(GC):
                    s = [np.zeros(n, dtype=np.int64) for _ in range(7)]
                    lp = trio_log_pmf(pad(gc), pad(GP[ip]), pad(GQ[iq]), KP, KQ, KP // 2, KQ // 2, 0.0, 0.0, ep, eq, logf,
                                      s[0], s[1], s[2], s[3], s[4], s[5], s[6], np.zeros(n))
                    x[j] = np.exp(lp)
                name = "part2_%dx%d_f%d_e%g_%g_p%d_q%d" % (KP, KQ, fi, ep, eq, ip, iq)
                names.append(name)
                out[name + "_shape"] = np.array([H, KP, KQ])
                out[name + "_case"] = np.array([fi, ep, eq, ip, iq])
                out[name + "_x"] = x
out["names"] = np.array(names)
np.savez_compressed(os.path.join(HERE, "cross_prior.npz"), **out)
print(len(names), "cases;", "sums", min(out[n + "_x"].sum() for n in names), max(out[n + "_x"].sum() for n in names),
      "; zeros", sum(int(np.sum(out[n + "_x"] == 0.0)) for n in names), "; nan", sum(int(np.sum(np.isnan(out[n + "_x"]))) for n in names))
