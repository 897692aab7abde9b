"""The expected read depth of every haplotype of one unit (call-exact --allele-depths) in long double, for the tests
of the support kernels and of the allele-depths file (tests/test_allele_support_reference.py, tests/test_gpu_allele_support_kernels.py,
tests/test_gpu_allele_depths.py):
    p[g]       = exp(llk[g] + lp[g]) / sum_g' exp(llk[g'] + lp[g'])
    D(r, g)    = sum_h c_h(g) P[r][h]
    post[r][h] = sum_g p[g] c_h(g) P[r][h] / D(r, g)        rows of weight 0: exactly 0
    depth[h]   = sum_r w_r post[r][h]
on tests/estimate_reference.py's genotype table and log prior (sums of logarithms, no lgamma; the prior's constant cancels in p),
with a plain loop over the genotypes.  The float64 host definition that ships, application.allele_support_unit, is held to it."""
import numpy as np

from tests.estimate_reference import LD, genotype_table, log_prior

# CPU-measured envelope of the float64 host definition against long double: the largest |float64 - long double| of an entry of
# depth divided by the unit's total read weight, and of an entry of a read's row (a row is a unit of weight 1)
# (tests/test_allele_support_reference.py measures, prints and asserts it) over tests/estimate_cases.py's tables and likelihoods
# formed from the drawn reads themselves: 8.75e-13 at `K10-H7`, 8.0e-13 at `K15-H6`, 3.4e-13 at `cut-run`, 1.7e-13 at
# `first-of-KM16`, 1.1e-13 at `K4-H17`, below 3e-14 at the other cases -- the loss is the prior's, the cancellation in
# lgamma(d + alpha) - lgamma(alpha) at large alpha, which also sets the envelopes of the model evidence and of the SNV posteriors
# (tests/evidence_reference.py, tests/snv_posterior_reference.py)
ENVELOPE = 9e-13
ENVELOPE_CASE = "K10-H7"
REL = 1e-9


def floor(weight):
    """FLOOR of the GPU tests' bound |got - want| <= REL |want| + FLOOR for a unit of total read weight `weight`: 8 times the
    envelope -- the project's margin for the device's lgamma / exp / log against libm, as tests/snv_posterior_reference.py --
    times the weight."""
    return 8.0 * ENVELOPE * weight


def draw_haplotypes(rng, H, M, A):
    """int8 [H, M]: H distinct haplotypes over A alleles at M positions (the first all reference)."""
    assert A ** M >= H
    seen = {(0,) * M}
    while len(seen) < H:
        seen.add(tuple(int(x) for x in rng.integers(0, A, size=M)))
    return np.array(sorted(seen), dtype=np.int8)


def draw_reads(rng, haps, R, A, error_free=False, error=0.01):
    """(dists float64 [R, M, A], counts int64 [R]): every row a read of one of `haps` with calls wrong at rate `error`, as the
    probabilities an encoder gives -- the called allele 1 - error, the others error / (A - 1); error_free: exactly 1 and exactly 0,
    and no wrong calls.  About a third of the positions of a row are gaps (NaN cells), every seventh row is all gaps, and the
    weights are drawn from 0..5 (row 0 keeps a weight, so the unit has one)."""
    H, M = haps.shape
    dists = np.empty((R, M, A))
    for r in range(R):
        true = haps[rng.integers(H)]
        for j in range(M):
            call = int(true[j])
            if not error_free and rng.random() < error:
                call = int((call + 1 + rng.integers(A - 1)) % A) if A > 1 else call
            dists[r, j] = (0.0 if error_free else error / max(A - 1, 1))
            dists[r, j, call] = 1.0 if error_free else 1.0 - error
            if rng.random() < 0.3:
                dists[r, j] = np.nan
        if r % 7 == 3:
            dists[r] = np.nan
    counts = rng.integers(0, 6, size=R).astype(np.int64)
    counts[0] = max(int(counts[0]), 1)
    return dists, counts


def products(dists, haps, dtype=LD):
    """[R, H]: P[r][h], the product over the non-NaN cells dists[r][j][haps[h][j]]."""
    d = np.asarray(dists, dtype=np.float64).astype(dtype)
    haps = np.asarray(haps, dtype=np.int64)
    P = np.ones((d.shape[0], len(haps)), dtype=dtype)
    for j in range(haps.shape[1]):
        v = d[:, j, :][:, haps[:, j]]
        P *= np.where(np.isnan(v), dtype(1), v)
    return P


def likelihoods(dists, counts, haps, K):
    """float64 [G]: the log likelihood of every genotype from the reads themselves, llk[g] = sum_r w_r log(sum_k P[r][g_k] / K), in
    float64 (-inf where a read with a weight fits no haplotype of the genotype)."""
    P = products(dists, haps, np.float64)
    g = genotype_table(len(haps), K)
    w = np.asarray(counts, dtype=np.float64)
    with np.errstate(divide="ignore"):
        lr = np.log(P[:, g].sum(axis=2) / K)   # [R, G]
    return (w[:, None] * np.where(w[:, None] > 0, lr, 0.0)).sum(axis=0)


def support(dists, counts, haps, llk, K, F, f):
    """(depth float64 [H], post float64 [R, H]): the definition in long double, rounded at the end; F None: the flat prior."""
    haps = np.asarray(haps, dtype=np.int64)
    H = len(haps)
    P = products(dists, haps)
    R = len(P)
    w = np.ones(R, dtype=LD) if counts is None else np.asarray(counts, dtype=np.float64).astype(LD)
    g = genotype_table(H, K)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lj = np.asarray(llk, dtype=np.float64).astype(LD)
        if F is not None:
            lj = lj + log_prior(g, H, K, F, f)
        m = np.max(lj)
        if not np.isfinite(m):
            return np.full(H, np.nan), np.full((R, H), np.nan)
        p = np.exp(lj - m)
        p = p / np.sum(p)
    post = np.zeros((R, H), dtype=LD)
    on = w > 0
    for gi in np.flatnonzero(p > 0):
        c = np.bincount(g[gi], minlength=H)              # the dosages of the genotype ...
        a = np.flatnonzero(c)                            # ... and its haplotypes
        c = c[a].astype(LD)
        Pa = P[:, a]
        D = Pa @ c
        ok = np.flatnonzero(on & (D > 0))
        post[np.ix_(ok, a)] += p[gi] * (Pa[ok] * c[None, :]) / D[ok, None]
    depth = (w[:, None] * post).sum(axis=0)
    return depth.astype(np.float64), post.astype(np.float64)


def within(got, want, weight):
    """(every entry within REL |want| + floor(weight) -- equal NaNs agree, a NaN where a number is wanted fails --, the largest
    |got - want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or np.any(np.isnan(got) != np.isnan(want)):
        return False, np.inf
    live = ~np.isnan(want)
    err = np.abs(got[live] - want[live])
    return bool(np.all(err <= REL * np.abs(want[live]) + floor(weight))), float(err.max()) if err.size else 0.0
