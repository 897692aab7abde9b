"""Inputs of the tests of `mchap call` over many known haplotypes (tests/test_call_wide.py, tests/test_gpu_call_wide.py)."""
import math

import numpy as np


def many_haplotypes(U, K, H, M, R, seed, qual=(5, 25)):
    """reads [U, R, M, 2] of `U` units of ploidy K over M biallelic SNVs and, per unit, H distinct known haplotypes [U, H, M] in
    random order, the unit's true haplotypes among them (H <= 2^M)."""
    from mchap_amd.synth import synth_units

    assert H <= 2 ** M
    rng = np.random.default_rng(seed)
    reads, _, truth = synth_units(U, ploidy=K, n_pos=M, n_reads=R, first_unit=seed, window=(2, M), qual=qual)
    weights = 1 << np.arange(M)
    haps = np.zeros((U, H, M), np.int8)
    for u in range(U):
        mine = np.unique(truth[u].astype(np.int64) @ weights)[:H]
        rest = np.setdiff1d(rng.permutation(2 ** M), mine, assume_unique=False)
        codes = np.concatenate([mine, rng.permutation(rest)[: H - len(mine)]])
        rng.shuffle(codes)
        haps[u] = ((codes[:, None] >> np.arange(M)[None, :]) & 1).astype(np.int8)
    return reads, haps


def wide_vcf(base_path, out_path, wide_records, seed=7):
    """The haplotype VCF `base_path` with one more record per (chrom, pos, id, n_alt) of `wide_records`, put in front of the
    base's record at that place: the same REF, the base record's ALT alleles first, then distinct random ones (SNVs at the base
    record's variable offsets and as many more as n_alt needs) up to n_alt."""
    rng = np.random.default_rng(seed)
    lines = [ln.rstrip("\n") for ln in open(base_path)]
    out = []
    for ln in lines:
        f = ln.split("\t")
        if not ln.startswith("#") and len(f) > 8:
            for chrom, pos, name, n_alt in wide_records:
                if (f[0], int(f[1])) != (chrom, pos):
                    continue
                ref = f[3]
                alts = [a for a in f[4].split(",") if a != "."]
                offsets = sorted({i for a in alts for i, (x, y) in enumerate(zip(a, ref)) if x != y})
                spare = [i for i in rng.permutation(len(ref)) if i not in offsets]
                while 4 ** len(offsets) < 2 * (n_alt + 1):
                    offsets.append(int(spare.pop()))
                seen = set(alts) | {ref}
                while len(alts) < n_alt:
                    s = list(ref)
                    for o in offsets:
                        s[o] = "ACGT"[int(rng.integers(0, 4))]
                    s = "".join(s)
                    if s not in seen:
                        seen.add(s)
                        alts.append(s)
                info = ";".join(kv for kv in f[7].split(";") if kv.split("=")[0] in ("END",))
                out.append("\t".join([chrom, str(pos), name, ref, ",".join(alts), ".", "PASS", info or ".", "GT"] + ["."] * (len(f) - 9)))
        out.append(ln)
    with open(out_path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def largest_haps_below_2_62(K):
    """the most haplotypes whose genotypes of ploidy K number less than 2^62 (the library's shape rule)"""
    lo, hi = 1, 1 << 32  # (bisection: 3 037 000 500 haplotypes at ploidy 2)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if math.comb(mid + K - 1, K) < 1 << 62:
            lo = mid
        else:
            hi = mid
    return lo


def rank_cases(K, H, n_random=300, seed=0):
    """sorted genotypes [n, K] over H haplotypes: the top one, the all-zero one, one allele apart from either, random ones over all
    alleles and random ones among the top few -- with their exact VCF indices as Python integers"""
    rng = np.random.default_rng(seed + 1000 * K + H)
    g = [np.full(K, H - 1), np.zeros(K, np.int64), np.append(np.zeros(K - 1, np.int64), H - 1), np.append(np.full(K - 1, H - 2), H - 1)]
    g += list(rng.integers(0, H, size=(n_random, K)))
    g += list(rng.integers(max(0, H - 8), H, size=(n_random // 4, K)))
    g = np.sort(np.array(g, dtype=np.int64), axis=1)
    exact = [sum(math.comb(int(a) + i, i + 1) for i, a in enumerate(row)) for row in g]
    return g, exact
