"""The selfing prior of one parent (call-exact --parentage-selfings) in long double and plain loops, straight from its
definition, for the tests of the host definition, of the selfing kernels and of the parentage table's selfing rows
(tests/test_selfing_reference.py, tests/test_gpu_selfing_kernels.py, tests/test_parentage_selfings_host.py):
    hyp(a | g)   = prod_h C(c_h(g), a_h) / C(K, t)                              t = K / 2
    gamma(a | g) = (1 - e) hyp(a | g) + e Mult(a; t, f)
    X(gc | g)    = sum_{a <= gc, |a| = t} gamma(a | g) gamma(gc - a | g)
    S[gc]        = sum_g p[g] X(gc | g)
    log_z        = log sum_gc S[gc] exp(llk_c[gc])
-- every genotype g, every ordered pair of its gametes with its full gamma: nothing of the expanded form the host definition and
the kernel take (application.selfing_prior) is used here.  The posterior p is tests/cross_reference.py's.  Also here: the shapes and the drawn
cases the CPU and the GPU tests share, and a synthetic block with a selfed progeny for application.MatrixSource."""
import functools
from math import comb, factorial

import numpy as np

from tests.cross_reference import BASES, F_POSITIVE, PARENT_KINDS, dosage, draw_frequencies, parent_llk, posterior
from tests.estimate_reference import LD, genotype_table

# CPU-measured envelope of the float64 host definition against long double: the largest |float64 - long double| of an entry of S
# over SHAPES below with every parent kind, prior and gamete error of unit_inputs (tests/test_selfing_reference.py measures, prints
# and asserts it).  The largest, 5.0e-16, is at `K4-H2` (a parent without reads, F > 0, e = 0): S there is the prior's own selfing
# distribution, entries near 0.3, and the loss is the prior's -- the cancellation in lgamma(d + alpha) - lgamma(alpha), as for the
# cross prior (tests/cross_reference.py); the sums themselves have few terms.
ENVELOPE = 1e-15
ENVELOPE_CASE = "K4-H2/no-reads/F+/e=0"
REL = 1e-9
FLOOR = 8.0 * ENVELOPE   # the project's margin for the device's lgamma / exp / log against libm

# name: (K, H) -- K in 2, 4, 6, 8, 14 with H from 2 to 5, each with every parent kind, prior and error of unit_inputs.  The sums cost
# G x NA^2 products (3060 x 330^2 at `K14-H5`): the tables that depend on the shape alone are formed once per shape.
SHAPES = {"K%d-H%d" % (K, H): (K, H) for K in (2, 4, 6, 8, 14) for H in (2, 3, 4, 5)}
ERRORS = (0.0, 0.01)


def mult(a, t, fl):
    """Mult(a; t, f) in long double."""
    coef = factorial(t)
    v = LD(1)
    for h, x in enumerate(a):
        coef //= factorial(x)
        v *= fl[h] ** x
    return LD(coef) * v


@functools.lru_cache(maxsize=4)
def hyp_rows(H, K):
    """longdouble [G, NA]: hyp(a | g) of every genotype and gamete (the shape's own: formed once)."""
    t = K // 2
    G, A = genotype_table(H, K), genotype_table(H, t)
    da = [dosage(a, H) for a in A]
    out = np.zeros((len(G), len(A)), dtype=LD)
    for j, g in enumerate(G):
        dg = dosage(g, H)
        for i, x in enumerate(da):
            w = 1
            for xh, ch in zip(x, dg):
                w *= comb(ch, xh)
            out[j, i] = LD(w) / LD(comb(K, t))
    return out


def gamma_rows(H, K, f, e):
    """longdouble [G, NA]: gamma(a | g) of every genotype and gamete."""
    t = K // 2
    fl = np.asarray(f, dtype=np.float64).astype(LD)
    m = np.array([mult(dosage(a, H), t, fl) for a in genotype_table(H, t)], dtype=LD)
    return (LD(1) - LD(e)) * hyp_rows(H, K) + LD(e) * m[None, :]


@functools.lru_cache(maxsize=4)
def pair_ranks(H, t):
    """int [NA, NA]: the VCF index of the genotype a + b."""
    A, GC = genotype_table(H, t), genotype_table(H, 2 * t)
    index = {tuple(int(x) for x in g): j for j, g in enumerate(GC)}
    return np.array([[index[tuple(sorted([int(x) for x in a] + [int(x) for x in b]))] for b in A] for a in A])


def selfing(p, H, K, f, e):
    """longdouble [G]: S from the posterior p (longdouble [G]); NaN throughout for a NaN posterior."""
    G = comb(H + K - 1, K)
    if np.any(np.isnan(p)):
        return np.full(G, np.nan, dtype=LD)
    rows, rank = gamma_rows(H, K, f, e), pair_ranks(H, K // 2)
    # pair[a][b] = sum_g p[g] gamma(a | g) gamma(b | g): the sum over g taken first, in long double throughout
    pair = np.dot(np.ascontiguousarray((rows * p[:, None]).T), rows)
    S = np.zeros(G, dtype=LD)
    for i in range(rows.shape[1]):
        S[rank[i]] += pair[i]   # (for one a the genotypes a + b are distinct)
    return S


def unit(llk, K, F, H, f, e, llk_c=None):
    """The definition in long double, rounded at the end: dict(S float64 [G], log_z)."""
    f = np.full(H, 1.0 / H) if f is None else f
    S = selfing(posterior(llk, H, K, F, f), H, K, f, e)
    out = dict(S=S.astype(np.float64))
    if llk_c is not None:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            m = np.max(np.asarray(llk_c, dtype=np.float64))
            out["log_z"] = float(LD(m) + np.log(np.sum(S * np.exp(np.asarray(llk_c, dtype=np.float64).astype(LD) - LD(m)))))
    return out


def unit_inputs(name, K, H):
    """The drawn cases of one shape: (label, llk, F, f, e, llk_c) over the parent kinds, the priors (flat; F = 0 with a zero
    frequency; F > 0) and ERRORS -- one seed per shape, the same on the CPU and the GPU."""
    rng = np.random.default_rng(sum(ord(c) for c in name) * 131 + 7)
    G = comb(H + K - 1, K)
    fr = draw_frequencies(rng, H)
    cases = []
    for kind in PARENT_KINDS:
        for prior, (F, f) in (("flat", (None, None)), ("F0-zero", (0.0, fr[0])), ("F+", (F_POSITIVE, fr[1]))):
            llk = parent_llk(rng, kind, G)
            if prior == "F0-zero" and kind == "one-hot":   # (the one possible genotype must be possible under the prior too)
                g = genotype_table(H, K)
                ok = [j for j in range(G) if all(fr[0][int(x)] > 0 for x in g[j])]
                llk = np.full(G, -np.inf)
                llk[ok[rng.integers(len(ok))]] = -3.0
            llk_c = -rng.exponential(4.0, size=G)
            for e in ERRORS:
                cases.append(("%s/%s/%s/e=%g" % (name, kind, prior, e), llk, F, f, e, llk_c))
    return cases


def selfing_block(seed=11, n_records=4, n_haps=(4, 3, 4), n_pos=6, depth=40, ploidy=4, min_distance=2):
    """A synthetic block for application.MatrixSource with a selfed progeny: (records, samples, matrices, truth).  Every record has
    its own haplotypes (as tests/cross_reference.py biparental_block); the samples are the parents P and Q with drawn genotypes, S0 a
    true self of P (two gametes of P, each drawn without replacement from its genotype), C0 a true P x Q progeny, and D0 a duplicate of
    P (P's genotype read again).  Reads: `depth` rows per sample and record, each a copy of one of the sample's haplotypes, one base
    in 200 wrong.  truth[(record index, sample)] = the genotype's ascending haplotype indices."""
    rng = np.random.default_rng(seed)
    t = ploidy // 2
    samples = ["P", "Q", "S0", "C0", "D0"]
    records, matrices, truth = [], {}, {}
    for ri in range(n_records):
        H = n_haps[ri % len(n_haps)]
        seen = ["A" * n_pos]
        while len(seen) < H:
            s = "".join(BASES[rng.integers(3)] for _ in range(n_pos))
            if s not in seen and all(sum(a != b for a, b in zip(s, u)) >= min_distance for u in seen):
                seen.append(s)
        var = [j for j in range(n_pos) if len({u[j] for u in seen}) > 1]
        rec = dict(chrom="chr1", pos=100 + 50 * ri, id="L%d" % ri, ref=seen[0], alts=tuple(seen[1:]), info={})
        records.append(rec)
        gp = sorted(int(x) for x in rng.integers(0, H, size=ploidy))
        gq = sorted(int(x) for x in rng.integers(0, H, size=ploidy))
        geno = {"P": gp, "Q": gq, "D0": list(gp)}
        geno["S0"] = sorted(list(rng.choice(gp, t, replace=False)) + list(rng.choice(gp, t, replace=False)))
        geno["C0"] = sorted(list(rng.choice(gp, t, replace=False)) + list(rng.choice(gq, t, replace=False)))
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
