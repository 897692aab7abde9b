"""The joint call of one nuclear family (call-exact --family-calls) in long double and direct sums, UNFACTORISED, for
the tests of the host definition and of the family kernels (tests/test_family_reference.py, tests/test_gpu_family_kernels.py):
    gamma_u(a | g) = (1 - e_u) prod_h C(c_h(g), a_h) / C(K_u, t_u) + e_u Mult(a; t_u, f)
    X(gc | gP, gQ) = sum_{a <= gc, |a| = t_P} gamma_P(a | gP) gamma_Q(gc - a | gQ)                     for every triple
    J(gP, gQ)      = exp(lp_P[gP] + llk_P[gP] + lp_Q[gQ] + llk_Q[gQ]) prod_c sum_gc X(gc | gP, gQ) exp(llk_c[gc])
    w = J / sum J,  post_P = sum_gQ w,  post_Q = sum_gP w
    q_c[gc]        = exp(llk_c[gc]) sum_{gP, gQ} (w / M_c)(gP, gQ) X(gc | gP, gQ),   M_c the progeny's factor of J
    pred_c         = -log sum_{gP, gQ} w / M_c
on tests/estimate_reference.py's genotype table and log prior (sums of logarithms, no lgamma; the prior's constant cancels in w), as
tests/cross_reference.py.  A progeny without reads (None) is left out of the product; its q_c takes w itself.  The float64 host
definition that ships, application.family_unit, is held to it."""
from math import comb, factorial

import numpy as np

from tests.cross_reference import dosage
from tests.estimate_reference import LD, genotype_table, log_prior

# CPU-measured envelope of application.family_unit against this file: the largest |float64 - long double| of a probability -- an
# entry of post_P, post_Q or of a q_c -- over the shapes CASES with every parent kind, prior, gamete error and progeny count of
# tests/test_family_reference.py, which measures, prints and asserts it.  The largest, 1.78e-15 (8 ulp of a probability near 1), is
# an entry of post_P at `2x2-H2` (random parents, F = 0, e = (0.01, 0.05), four progeny): the logarithm of each progeny's factor
# and the exponential of their sum each round once, and the sum's error enters the exponential absolutely.  ENVELOPE is that value
# with the head-room tests/cross_reference.py leaves (half as much again, rounded up).
MEASURED = 1.78e-15
ENVELOPE = 3e-15
ENVELOPE_CASE = "2x2-H2"
REL = 1e-9
FLOOR = 8.0 * ENVELOPE   # the project's margin for the device's lgamma / exp / log against libm (tests/cross_reference.within)

# name: (K_P, K_Q, H)
CASES = {
    "2x2-H2": (2, 2, 2),
    "2x2-H5": (2, 2, 5),
    "4x4-H3": (4, 4, 3),
    "4x4-H4": (4, 4, 4),
    "4x2-H4": (4, 2, 4),
    "6x6-H3": (6, 6, 3),
    "8x8-H3": (8, 8, 3),
}


def gamma_rows(H, K, f, e):
    """longdouble [G, NA]: gamma(a | g) for every genotype g of ploidy K and every gamete a of K / 2 haplotypes."""
    t = K // 2
    G, A = genotype_table(H, K), genotype_table(H, t)
    fl = np.asarray(f, dtype=np.float64).astype(LD)
    out = np.zeros((len(G), len(A)), dtype=LD)
    for i, a in enumerate(A):
        da = dosage(a, H)
        coef = factorial(t)
        mult = LD(1)
        for h, x in enumerate(da):
            coef //= factorial(x)
            mult *= fl[h] ** x
        for j, g in enumerate(G):
            w = 1
            for x, c in zip(da, dosage(g, H)):
                w *= comb(c, x)
            out[j, i] = (LD(1) - LD(e)) * (LD(w) / LD(comb(K, t))) + LD(e) * (LD(coef) * mult)
    return out


def transmission(gam_p, gam_q, H, tp, tq):
    """longdouble [G_P, G_Q, G_c]: X(gc | gP, gQ) for every triple, from its definition."""
    A, GC = genotype_table(H, tp), genotype_table(H, tp + tq)
    index_q = {tuple(int(x) for x in b): i for i, b in enumerate(genotype_table(H, tq))}
    da = [dosage(a, H) for a in A]
    X = np.zeros((gam_p.shape[0], gam_q.shape[0], len(GC)), dtype=LD)
    for j, gc in enumerate(GC):
        dc = dosage(gc, H)
        for i in range(len(A)):
            if all(x <= c for x, c in zip(da[i], dc)):
                b = tuple(h for h in range(H) for _ in range(dc[h] - da[i][h]))
                X[:, :, j] += np.outer(gam_p[:, i], gam_q[:, index_q[b]])   # (every (gP, gQ) of the triple, one product each)
    return X


def family(llk_p, K_p, F_p, llk_q, K_q, F_q, H, f, errors, llk_progeny, X=None):
    """The definition in long double by direct sums, rounded at the end: dict(post_p, post_q, q [n][G_c], pred [n]) of float64
    arrays; all NaN where sum J is 0 or not a number.  X: transmission() of the same (shape, f, errors), where the caller kept it."""
    f = np.full(H, 1.0 / H) if f is None else f
    if X is None:
        X = transmission(gamma_rows(H, K_p, f, errors[0]), gamma_rows(H, K_q, f, errors[1]), H, K_p // 2, K_q // 2)
    GP, GQ, GC = X.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a_p = np.asarray(llk_p, dtype=np.float64).astype(LD)
        a_q = np.asarray(llk_q, dtype=np.float64).astype(LD)
        if F_p is not None:
            a_p = a_p + log_prior(genotype_table(H, K_p), H, K_p, F_p, f)
        if F_q is not None:
            a_q = a_q + log_prior(genotype_table(H, K_q), H, K_q, F_q, f)
        a_p, a_q = a_p - np.max(a_p), a_q - np.max(a_q)
        J = np.outer(np.exp(a_p), np.exp(a_q))
        Ms = []
        for llk in llk_progeny:
            if llk is None:
                Ms.append(None)
                continue
            lc = np.asarray(llk, dtype=np.float64).astype(LD)
            lc = lc - np.max(lc)
            M = np.tensordot(X, np.exp(lc), axes=([2], [0]))   # (long double has no BLAS: numpy's own loops, term by term)
            J = J * M
            Ms.append((M, lc, np.max(np.asarray(llk, dtype=np.float64).astype(LD))))
        z = np.sum(J)
        n = len(llk_progeny)
        if not (z > 0) or not np.isfinite(z):
            nan = np.nan
            return dict(post_p=np.full(GP, nan), post_q=np.full(GQ, nan), q=[np.full(GC, nan) for _ in range(n)], pred=np.full(n, nan))
        w = J / z
        q, pred = [], np.zeros(n)
        for c, fac in enumerate(Ms):
            if fac is None:
                d, scale = w, np.ones(GC, dtype=LD)
            else:
                M, lc, m = fac
                d = np.where(w == 0, LD(0), w / np.where(M == 0, LD(1), M))
                scale = np.exp(lc)
                pred[c] = float(m - np.log(np.sum(d)))
            q.append((scale * np.tensordot(d, X, axes=([0, 1], [0, 1]))).astype(np.float64))
    return dict(post_p=np.sum(w, axis=1).astype(np.float64), post_q=np.sum(w, axis=0).astype(np.float64), q=q, pred=pred)
