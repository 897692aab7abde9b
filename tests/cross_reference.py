"""The cross prior of one trio (call-exact --cross-calls) in long double and plain loops, for the tests of the host
definition, of the cross kernels and of the cross-calls file (tests/test_cross_prior_reference.py, tests/test_gpu_cross_kernels.py,
tests/test_cross_calls_host.py, tests/test_gpu_cross_calls.py):
    p[g]    = exp(llk[g] + lp[g]) / sum_g' exp(llk[g'] + lp[g'])                 the parent's posterior under its calling prior
    gam[a]  = sum_{g >= a} p[g] prod_h C(c_h(g), a_h) / C(K, t)                  t = K / 2
    gam'[a] = (1 - e) gam[a] + e Mult(a; t, f)
    X[gc]   = sum_{a <= gc, |a| = t_P} gam'_P[a] gam'_Q[gc - a]
    q[gc]   = X[gc] exp(llk_c[gc]) / Z
on tests/estimate_reference.py's genotype table and log prior (sums of logarithms, no lgamma; the prior's constant cancels in p).
The float64 host definition that ships, application.cross_prior_unit, is held to it.  Also here: the drawn cases the CPU and the
GPU tests share, a float64 numpy likelihood backend, and a synthetic bi-parental block for application.MatrixSource."""
from math import comb, factorial

import numpy as np

from tests.estimate_reference import LD, genotype_table, log_prior

# CPU-measured envelope of the float64 host definition against long double: the largest |float64 - long double| of a probability
# -- an entry of a gamete table, of X, of q -- over CASES below with every parent kind, prior and gamete error of trio_inputs
# (tests/test_cross_prior_reference.py measures, prints and asserts it).  The largest, 1.33e-15, is an entry of a gamete table at
# `14x14-H2` (random parents, F > 0, e = 0): the loss is the prior's, the cancellation in lgamma(d + alpha) - lgamma(alpha), as for
# the allele support (tests/allele_support_reference.py); the sums themselves have few terms.
ENVELOPE = 2e-15
ENVELOPE_CASE = "14x14-H2"
REL = 1e-9
FLOOR = 8.0 * ENVELOPE   # the project's margin for the device's lgamma / exp / log against libm

# name: (K_P, K_Q, H) -- the shapes the CPU reference walks in plain loops
CASES = {
    "2x2-H2": (2, 2, 2),
    "2x2-H5": (2, 2, 5),
    "4x4-H3": (4, 4, 3),
    "4x4-H4": (4, 4, 4),
    "4x2-H4": (4, 2, 4),
    "6x6-H4": (6, 6, 4),
    "8x8-H3": (8, 8, 3),
    "10x8-H3": (10, 8, 3),
    "14x14-H2": (14, 14, 2),
}
PARENT_KINDS = ("random", "one-hot", "no-reads")
F_POSITIVE = 0.3


def dosage(t, H):
    d = [0] * H
    for x in t:
        d[int(x)] += 1
    return d


def posterior(llk, H, K, F, f):
    """longdouble [G]: the unit's posterior under its calling prior (F None: flat); NaN without a finite genotype."""
    g = genotype_table(H, K)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lj = np.asarray(llk, dtype=np.float64).astype(LD)
        if F is not None:
            lj = lj + log_prior(g, H, K, F, f)
        m = np.max(lj)
        if not np.isfinite(m):
            return np.full(len(lj), np.nan, dtype=LD)
        p = np.exp(lj - m)
        return p / np.sum(p)


def gametes(p, H, K, f, e):
    """longdouble [C(H + t - 1, t)]: the gamete table of a parent with posterior p, mixed with Mult(.; t, f) at error e."""
    t = K // 2
    G, A = genotype_table(H, K), genotype_table(H, t)
    dg = [dosage(g, H) for g in G]
    out = np.zeros(len(A), dtype=LD)
    fl = np.asarray(f, dtype=np.float64).astype(LD)
    for i, a in enumerate(A):
        da = dosage(a, H)
        total = LD(0)
        for j in range(len(G)):
            if all(x <= c for x, c in zip(da, dg[j])):
                w = 1
                for x, c in zip(da, dg[j]):
                    w *= comb(c, x)
                total += p[j] * LD(w)
        coef = factorial(t)
        mult = LD(1)
        for h, x in enumerate(da):
            coef //= factorial(x)
            mult *= fl[h] ** x
        out[i] = (LD(1) - LD(e)) * (total / LD(comb(K, t))) + LD(e) * (LD(coef) * mult)
    return out


def cross(gam_p, gam_q, H, tp, tq):
    """longdouble [G_c]: X from the two gamete tables."""
    A, GC = genotype_table(H, tp), genotype_table(H, tp + tq)
    index_q = {tuple(int(x) for x in b): i for i, b in enumerate(genotype_table(H, tq))}
    da = [dosage(a, H) for a in A]
    X = np.zeros(len(GC), dtype=LD)
    for j, gc in enumerate(GC):
        dc = dosage(gc, H)
        for i in range(len(A)):
            if all(x <= c for x, c in zip(da[i], dc)):
                b = tuple(h for h in range(H) for _ in range(dc[h] - da[i][h]))
                X[j] += gam_p[i] * gam_q[index_q[b]]
    return X


def trio(llk_p, K_p, F_p, llk_q, K_q, F_q, H, f, errors, llk_c):
    """The definition in long double, rounded at the end: dict(gam_p, gam_q, X, q) of float64 arrays."""
    f = np.full(H, 1.0 / H) if f is None else f
    gp = gametes(posterior(llk_p, H, K_p, F_p, f), H, K_p, f, errors[0])
    gq = gametes(posterior(llk_q, H, K_q, F_q, f), H, K_q, f, errors[1])
    X = cross(gp, gq, H, K_p // 2, K_q // 2)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = X * np.exp(np.asarray(llk_c, dtype=np.float64).astype(LD))
        z = np.sum(t)
        q = t / z if z > 0 else np.full(len(t), np.nan, dtype=LD)
    return dict(gam_p=gp.astype(np.float64), gam_q=gq.astype(np.float64), X=X.astype(np.float64), q=q.astype(np.float64))


def parent_llk(rng, kind, G):
    """float64 [G]: the likelihoods of a parent of `kind` -- drawn, all but one genotype impossible, or no reads at all."""
    if kind == "random":
        return -rng.exponential(4.0, size=G)
    if kind == "one-hot":
        llk = np.full(G, -np.inf)
        llk[rng.integers(G)] = -3.0
        return llk
    return np.zeros(G)


def draw_frequencies(rng, H, rows=3):
    """float64 [rows, H]: drawn frequency rows, row 0 with a zero frequency."""
    fr = rng.dirichlet(np.full(H, 2.0), size=rows)
    fr[0, 1 % H] = 0.0
    fr[0] /= fr[0].sum()
    return fr


def within(got, want, floor=FLOOR):
    """(every entry within REL |want| + floor -- equal NaNs agree, exact zeros must be exact zeros --, the largest |got - want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or np.any(np.isnan(got) != np.isnan(want)) or np.any((got == 0.0) != (want == 0.0)):
        return False, np.inf
    live = ~np.isnan(want)
    err = np.abs(got[live] - want[live])
    return bool(np.all(err <= REL * np.abs(want[live]) + floor)), float(err.max()) if err.size else 0.0


class NumpyBackend:
    """genotype_likelihoods of the reads themselves in float64 numpy: llk[g] = sum_r w_r log(sum_k P[r][g_k] / K), P[r][h] the
    product over the non-NaN cells of row r at haplotype h -- what the exact caller computes, as a host backend for the writers."""

    def genotype_likelihoods(self, dists, ploidy, haplotypes, read_counts=None):
        d = np.asarray(dists, dtype=np.float64)
        haps = np.asarray(haplotypes, dtype=np.int64)
        P = np.ones((d.shape[0], len(haps)))
        for j in range(haps.shape[1]):
            v = d[:, j, :][:, haps[:, j]]
            P *= np.where(np.isnan(v), 1.0, v)
        g = genotype_table(len(haps), ploidy)
        w = np.ones(len(d)) if read_counts is None else np.asarray(read_counts, dtype=np.float64)
        with np.errstate(divide="ignore"):
            lr = np.log(P[:, g].sum(axis=2) / ploidy)
        return (w[:, None] * np.where(w[:, None] > 0, lr, 0.0)).sum(axis=0)


BASES = "ACGT"


def biparental_block(seed=7, n_records=3, n_haps=(4, 3, 5), n_pos=5, depth=60, n_progeny=3, ploidy_p=4, ploidy_q=4, extra=None,
                     min_distance=2):
    """A synthetic bi-parental block for application.MatrixSource: (records, samples, matrices, truth).  Every record has its own
    haplotypes (n_haps[i] of them, n_pos bases, the first the reference, any two at least min_distance bases apart); the samples are the parents P and Q with drawn
    genotypes, n_progeny progeny C0.. of the cross (one gamete of each parent, drawn without replacement from its genotype), an
    unrelated sample U0 of the progeny's ploidy, drawn from the haplotypes the parents do NOT carry where there are any, and the
    samples of `extra` {name: ploidy} with drawn genotypes.  Reads: `depth` rows per sample and record, each a copy of one of
    the sample's haplotypes, one base in 200 wrong.  truth[(record index, sample)] = the genotype's ascending haplotype indices."""
    rng = np.random.default_rng(seed)
    kc = ploidy_p // 2 + ploidy_q // 2
    samples = ["P", "Q"] + ["C%d" % i for i in range(n_progeny)] + ["U0"] + list(extra or {})
    records, matrices, truth = [], {}, {}
    for ri in range(n_records):
        H = n_haps[ri % len(n_haps)]
        seen = ["A" * n_pos]
        while len(seen) < H:
            s = "".join(BASES[rng.integers(3)] for _ in range(n_pos))
            if s not in seen and all(sum(a != b for a, b in zip(s, t)) >= min_distance for t in seen):
                seen.append(s)
        var = [j for j in range(n_pos) if len({t[j] for t in seen}) > 1]   # (a pileup matrix has the variable positions alone)
        rec = dict(chrom="chr1", pos=100 + 50 * ri, id="L%d" % ri, ref=seen[0], alts=tuple(seen[1:]), info={})
        records.append(rec)
        gp = sorted(int(x) for x in rng.integers(0, max(H - 1, 1), size=ploidy_p))
        gq = sorted(int(x) for x in rng.integers(0, max(H - 1, 1), size=ploidy_q))
        geno = {"P": gp, "Q": gq}
        for i in range(n_progeny):
            geno["C%d" % i] = sorted(list(rng.choice(gp, ploidy_p // 2, replace=False)) + list(rng.choice(gq, ploidy_q // 2, replace=False)))
        geno["U0"] = [H - 1] * kc                       # (the parents are drawn from the haplotypes below the last)
        for s, k in (extra or {}).items():
            geno[s] = sorted(int(x) for x in rng.integers(0, H, size=k))
        for s in samples:
            truth[(ri, s)] = tuple(int(x) for x in geno[s])
            rows = []
            for _ in range(depth):
                read = list(seen[geno[s][rng.integers(len(geno[s]))]])
                for j in range(n_pos):
                    if rng.random() < 0.005:
                        read[j] = BASES[(BASES.index(read[j]) + 1 + rng.integers(2)) % 3]
                rows.append([read[j] for j in var])
            matrices[(rec["id"], s)] = (np.array(rows), np.full((depth, len(var)), 30, dtype=np.int16))
    return records, samples, matrices, truth
