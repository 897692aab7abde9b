"""Synthetic blocks of call-exact records for the tests of the prior allele-frequency estimate (tests/test_estimate_frequencies.py,
tests/test_gpu_estimate_frequencies.py): units as application._exact_units returns them, built from drawn reads instead of
files, and an independent brute-force iteration in float64."""
import itertools
import math
from types import SimpleNamespace

import numpy as np


def make_record(rng, H, M, ploidies, n_reads, masked=False, f0=None, error=0.01, name="r"):
    """One record as a unit of application._exact_units: H distinct biallelic haplotypes over M positions; per sample (ploidy
    ploidies[s], n_reads[s] reads, 0 = a sample without reads) reads drawn from a random genotype, every third one with a gap,
    de-duplicated into distinct rows with counts."""
    assert H <= 2 ** M
    codes = rng.choice(2 ** M, size=H, replace=False)
    haps = ((codes[:, None] >> np.arange(M)[None, :]) & 1).astype(np.int8)
    f = np.full(H, 1.0 / H) if f0 is None else np.array(f0, dtype=np.float64)
    if masked:
        f[0] = 0.0
    f = f / f.sum()
    reads = {}
    for s, (K, R) in enumerate(zip(ploidies, n_reads)):
        geno = rng.integers(1 if masked else 0, H, size=K)
        rows = []
        for r in range(R):
            row = haps[geno[rng.integers(K)]].astype(np.int64).copy()
            flip = rng.random(M) < error
            row[flip] = 1 - row[flip]
            if r % 3 == 2:
                row[rng.integers(M)] = -1
            rows.append(row)
        calls = np.array(rows, dtype=np.int8).reshape(R, M)
        if R:
            ucalls, counts = np.unique(calls, axis=0, return_counts=True)
        else:
            ucalls, counts = calls, np.zeros(0, dtype=np.int64)
        dists = np.full((len(ucalls), M, 2), np.nan)
        for a in (0, 1):
            dists[:, :, a] = np.where(ucalls == a, 1.0 - error, error)
        dists[ucalls < 0] = np.nan
        reads["S%d" % s] = dict(dists=dists, counts=counts.astype(np.int64), calls=calls, depth=np.full(M, float(R)))
    locus = SimpleNamespace(haplotypes=haps, frequencies=f, n_alleles=[2] * M, mask_reference_allele=masked, name=name)
    return dict(rec=dict(chrom="c", pos=1, id=name), locus=locus, invalid=None, reads=reads, needs_kernel=True, block=None, li=0)


def fresh(units):
    """A copy of the units whose loci carry their own frequency rows (the estimate replaces them)."""
    out = []
    for u in units:
        l = u["locus"]
        v = dict(u)
        v["locus"] = SimpleNamespace(**{**vars(l), "frequencies": np.array(l.frequencies)})
        out.append(v)
    return out


def samples_of(units):
    return list(units[0]["reads"])


def per_sample(values):
    return lambda s: values[int(s[1:])]


def brute_sample_frequencies(dists, counts, haps, K, F, f):
    """Mean posterior allele frequencies of one sample under the Dirichlet-multinomial prior (F, f), over every multiset of K
    haplotypes: plain float64, math.lgamma."""
    H = len(haps)
    f = np.asarray(f, dtype=np.float64)
    alpha = f * (1.0 - F) / F if F > 0 else None   # (F = 0: the multinomial prior over the frequencies themselves)
    lj, dos = [], []
    for g in itertools.combinations_with_replacement(range(H), K):
        llk = 0.0
        for r in range(len(dists)):
            tot = 0.0
            for h in g:
                p = 1.0
                for j in range(dists.shape[1]):
                    v = dists[r, j, haps[h, j]]
                    if not np.isnan(v):
                        p *= v
                tot += p / K
            llk += math.log(tot) * counts[r]
        d = np.bincount(g, minlength=H)
        lp = math.lgamma(K + 1) + (math.lgamma(alpha.sum()) - math.lgamma(K + alpha.sum()) if F > 0 else 0.0)
        for h in range(H):
            if d[h] == 0:
                continue
            if f[h] == 0.0:
                lp = -math.inf
                break
            if F > 0:
                lp += math.lgamma(d[h] + alpha[h]) - math.lgamma(d[h] + 1) - math.lgamma(alpha[h])
            else:
                lp += d[h] * math.log(f[h]) - math.lgamma(d[h] + 1)
        lj.append(llk + lp)
        dos.append(d)
    lj = np.array(lj)
    p = np.exp(lj - lj.max())
    p /= p.sum()
    return (p[:, None] * np.array(dos)).sum(axis=0) / K


def brute_iterate(unit, ploidies, inbreeding, n):
    """f_1 .. f_n of one record by the definition: f' = sum_s K_s freqs_s(f) / sum_s K_s."""
    f = np.array(unit["locus"].frequencies, dtype=np.float64)
    out = []
    for _ in range(n):
        acc = np.zeros(len(f))
        for s, sr in unit["reads"].items():
            K, F = ploidies[int(s[1:])], inbreeding[int(s[1:])]
            acc += K * brute_sample_frequencies(sr["dists"], sr["counts"], unit["locus"].haplotypes, K, F, f)
        f = acc / float(sum(ploidies))
        out.append(f)
    return out


def close(a, b, rel, floor=1e-12):
    """max |a - b| within rel * |b| + floor, elementwise; returns the largest excess ratio for printing."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= rel * np.abs(b) + floor)), float(np.max(np.abs(a - b)))
