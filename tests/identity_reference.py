"""The identity evidence of one record (call-exact --identity) in long double and plain loops, for the tests of the
host definition and of the identity kernels (tests/test_identity_reference.py, tests/test_gpu_identity_kernels.py):
    lbf[i][j] = log((1 - e) r_ij + e),  r_ij = sum_g pi(g) L_i(g) L_j(g) / (Z_i Z_j),
pair by pair, with the one clause of the definition: the scaled sum sum_g a_i(g) a_j(g), a_s(g) = exp(llk_s(g) + log pi(g) / 2 -
m_s), below 1e-290 counts as 0.  The float64 host definition that ships, application.identity_unit, is held to it.  Also here:
the shapes, the drawn likelihoods and the bound the CPU and the GPU tests share."""
import zlib
from math import comb

import numpy as np

from mchap_amd import application
from tests.estimate_reference import LD

TINY = 1e-290
REL = 1e-9
# (ploidy, haplotypes): G = 5, 6, 35 (not a multiple of 4), 462, 3876 (two chunks of the genotype axis: a chunk holds 2048 at least)
SHAPES = [(1, 5), (2, 3), (4, 4), (6, 6), (4, 16)]
PRIORS = [None, 0.0, 0.3]     # the flat prior, F = 0, F = 0.3
PEAK = 2000.0                 # nats between the two peaked rows' best and other genotypes


def floor(G):
    """The absolute part of the bound on a term: a sum of G positive float64 terms, each a product of two exp with arguments up to
    about 745 in size; log((1 - e) r + e) does not expand an error in log r."""
    return (G + 4096) * 2.0 ** -52


def log_prior(K, H, F, f):
    return application._host_log_prior(application._genotype_table(H, K), H, K, F, f)


def lbf(llks, lp, error, reads=None):
    """float64 [n, n]: the definition in long double, rounded at the end; the diagonal NaN.  A sample without reads: exactly 0; one
    with reads without a finite llk + log pi, or with a NaN: NaN in its row and column."""
    A = np.atleast_2d(np.asarray(llks, dtype=np.float64)).astype(LD)
    lp = np.asarray(lp, dtype=np.float64).astype(LD)
    n = len(A)
    e = LD(error)
    has = [True] * n if reads is None else [bool(x) for x in reads]
    out = np.full((n, n), np.nan)
    a, c, bad = [None] * n, [LD(0)] * n, [False] * n
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for s in range(n):
            if not has[s]:
                continue
            w = A[s] + lp / 2
            full = A[s] + lp
            if np.any(np.isnan(w)) or not np.any(np.isfinite(w)):
                bad[s] = True
                continue
            m, mz = np.max(w), np.max(full)
            a[s] = np.exp(w - m)
            c[s] = m - (mz + np.log(np.sum(np.exp(full - mz))))
        for i in range(n):
            for j in range(n):
                if i == j or bad[i] or bad[j]:
                    continue
                if not has[i] or not has[j]:
                    out[i, j] = 0.0
                    continue
                S = np.sum(a[i] * a[j])
                if S < TINY:
                    S = LD(0)
                lr = np.log(S) + (c[i] + c[j])
                out[i, j] = float(lr) if error == 0 else float(np.log((1 - e) * np.exp(lr) + e))
    return out


def draw_case(K, H, n, records=3):
    """The drawn inputs of a shape: (llk [records, n, G], reads [records, n] of 0 / 1, f [records, H]).  Likelihoods
    -exponential(4); record 0 is under a zero frequency and holds, from two samples on, two rows peaked PEAK nats apart on
    different genotypes (the first and the last row: the clause); record 1 holds a sample without reads (sample 1 % n; its
    likelihoods are NaN here: they are not to be looked at), record 2 a sample whose likelihoods are all -inf (sample 2 % n).
    From 17 samples on record 1 also has a sample without a finite genotype (5) beside the one without reads, and peaked rows (7, 11)."""
    rng = np.random.default_rng(zlib.crc32(("identity-%d-%d-%d-%d" % (K, H, n, records)).encode()))
    G = comb(H + K - 1, K)
    fr = rng.dirichlet(np.full(H, 2.0), size=records)
    fr[0, 1 % H] = 0.0
    fr[0] /= fr[0].sum()
    llk = -rng.exponential(4.0, size=(records, n, G))
    reads = np.ones((records, n), dtype=np.int32)

    def peak(r, s, g):
        llk[r, s] = -PEAK
        llk[r, s, g] = 0.0

    if n >= 2:
        peak(0, 0, 0)
        peak(0, n - 1, G - 1)
    if records > 1:
        reads[1, 1 % n] = 0
        llk[1, 1 % n] = np.nan
    if records > 2:
        llk[2, 2 % n] = -np.inf
    if n >= 17 and records > 1:
        llk[1, 5] = -np.inf
        peak(1, 7, 0)
        peak(1, 11, G - 1)
    return llk, reads, fr


def within(got, want, G):
    """(every entry within REL |want| + floor(G) -- NaN, -inf and the exact 0 must match exactly --, the largest |got - want| of the
    finite)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or np.any(np.isnan(got) != np.isnan(want)) or np.any(np.isinf(got) != np.isinf(want)):
        return False, np.inf
    if np.any(got[np.isinf(want)] != want[np.isinf(want)]) or np.any((got == 0.0) != (want == 0.0)):
        return False, np.inf
    live = np.isfinite(want)
    err = np.abs(got[live] - want[live])
    return bool(np.all(err <= REL * np.abs(want[live]) + floor(G))), float(err.max()) if err.size else 0.0


PANEL = dict(seed=7, n_records=6, depth=60, extra={"X0": 4, "X2": 2, "X3": 2})
DUPLICATE = ("P", "P_again")


def panel(**kw):
    """A simulated panel for application.MatrixSource (tests/cross_reference.py biparental_block): (records, samples, matrices,
    ploidy_of).  Tetraploids P, Q, C0..C2, U0, X0 and the diploids X2, X3 -- and P_again, a second name for P: the two share P's
    genotype at every record and split its reads, 30 rows each."""
    from tests import cross_reference

    records, samples, matrices, _ = cross_reference.biparental_block(**dict(PANEL, **kw))
    extra = dict(PANEL, **kw)["extra"]
    for rec in records:
        calls, quals = matrices[(rec["id"], "P")]
        half = len(calls) // 2
        matrices[(rec["id"], "P")] = (calls[:half], quals[:half])
        matrices[(rec["id"], DUPLICATE[1])] = (calls[half:], quals[half:])
    return records, samples + [DUPLICATE[1]], matrices, lambda s: extra.get(s, 4)
