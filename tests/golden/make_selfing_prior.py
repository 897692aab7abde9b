#!/usr/bin/env python3
"""Generate tests/golden/selfing_prior.npz: what the reference gives for the genotype distribution of a selfed parent's progeny, as
arrays in VCF order (mchap/pedigree/prior.py trio_log_pmf with the SAME genotype as both parents and lambda = 0): exp of the log
pmf of every progeny genotype, for ploidy 2, 4, 6 and 8 over 3 haplotypes, three drawn parental genotypes and one homozygote per
ploidy, gamete errors 0, 0.01 and 0.2, a drawn frequency row and one with a zero.  Also per ploidy one drawn posterior p over the
parental genotypes, with some exact zeros, and sum_g p[g] X(. | g) formed from the reference's values for every genotype, per
frequency row and error.  The reference is imported under the identity shims of tests/golden/_shim.  Build container only (needs
/root/reference); the output is data, not source.
Usage: python tests/golden/make_selfing_prior.py"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")

from mchap.pedigree.prior import trio_log_pmf  # noqa: E402


def table(H, K):
    """The ascending multisets of K out of H in VCF order."""
    return sorted(itertools.combinations_with_replacement(range(H), K), key=lambda t: t[::-1])


def selfed(G, ig, K, e, logf):
    """exp(trio_log_pmf(gc, g, g, ...)) for every gc."""
    g = np.array(G[ig], dtype=np.int64)
    x = np.zeros(len(G))
    for j, gc in enumerate(G):
        s = [np.zeros(K, dtype=np.int64) for _ in range(7)]
        x[j] = np.exp(trio_log_pmf(np.array(gc, dtype=np.int64), g.copy(), g.copy(), K, K, K // 2, K // 2, 0.0, 0.0, e, e, logf,
                                   s[0], s[1], s[2], s[3], s[4], s[5], s[6], np.zeros(K)))
    return x


rng = np.random.default_rng(20261022)
H = 3
freqs = np.stack([rng.dirichlet(np.full(H, 2.0)), np.array([0.6, 0.0, 0.4])])
out = {"freqs": freqs}
names, mixes = [], []
for K in (2, 4, 6, 8):
    G = table(H, K)
    picks = [int(i) for i in rng.choice(len(G), 3, replace=False)] + [G.index((1,) * K)]
    p = rng.dirichlet(np.ones(len(G)))
    p[rng.random(len(G)) < 0.4] = 0.0
    p[picks[0]] += 1e-3
    p /= p.sum()
    out["mix_K%d_p" % K] = p
    for fi in range(len(freqs)):
        with np.errstate(divide="ignore"):
            logf = np.log(freqs[fi])
        for e in (0.0, 0.01, 0.2):
            rows = np.stack([selfed(G, ig, K, e, logf) for ig in range(len(G))])
            for ig in picks:
                name = "K%d_f%d_e%g_g%d" % (K, fi, e, ig)
                names.append(name)
                out[name + "_case"] = np.array([K, fi, e, ig])
                out[name + "_x"] = rows[ig]
            mix = np.zeros(len(G))
            for ig in range(len(G)):   # (in genotype order, one term after the other)
                mix += p[ig] * rows[ig]
            name = "mix_K%d_f%d_e%g" % (K, fi, e)
            mixes.append(name)
            out[name + "_case"] = np.array([K, fi, e])
            out[name + "_s"] = mix
out["names"], out["mixes"] = np.array(names), np.array(mixes)
np.savez_compressed(os.path.join(HERE, "selfing_prior.npz"), **out)
sums = [out[n + "_x"].sum() for n in names if not (out[n + "_case"][2] == 0.0 and out[n + "_x"].sum() == 0.0)]
print(len(names), "cases,", len(mixes), "mixtures; sums", min(sums), max(sums),
      "; zeros", sum(int(np.sum(out[n + "_x"] == 0.0)) for n in names), "; nan", sum(int(np.sum(np.isnan(out[n + "_x"]))) for n in names))
