"""The parentage evidence of one progeny (call-exact --parentage) in long double and plain loops, for the tests of the
host definition, of the parentage kernels and of the parentage table (tests/test_parentage_reference.py,
tests/test_gpu_parentage_kernels.py, tests/test_parentage_host.py, tests/test_gpu_parentage.py):
    log_z[i][j] = log sum_a sum_b gam_a[i][a] gam_b[j][b] exp(llk_c[rank(a + b)])
over every pair (a, b) of a gamete of t_a and a gamete of t_b haplotypes: unrank both, merge, rank, add.  The float64 host
definition that ships, application.parentage_unit, is held to it.  Also here: the shapes and the drawn tables the CPU and the GPU
tests share."""
import zlib
from math import comb

import numpy as np

from mchap_amd import application
from tests.estimate_reference import LD

# CPU-measured envelope of the float64 host definition against long double: the largest |float64 - long double| of a finite log
# evidence over SHAPES below with the three rows and three progeny of draw_case (tests/test_parentage_reference.py measures, prints
# and asserts it).  The largest, 8.88e-16, is at `1x1-H2` and is one unit in the last place of a value between 4 and 8: the terms
# are of one sign, so the sums lose nothing, and what is left is the rounding of m + log z itself.
ENVELOPE = 1e-15
ENVELOPE_CASE = "1x1-H2"
REL = 1e-9
FLOOR = 8.0 * ENVELOPE   # the project's margin for the device's exp / log against libm

# name: (t_a, t_b, H)
SHAPES = {
    "1x1-H2": (1, 1, 2),
    "1x1-H91": (1, 1, 91),
    "2x2-H3": (2, 2, 3),
    "2x2-H22": (2, 2, 22),     # 253 gametes: one tile of rows
    "2x2-H23": (2, 2, 23),     # 276: the second tile
    "2x1-H4": (2, 1, 4),       # a triploid progeny, both orientations
    "1x2-H4": (1, 2, 4),
    "4x4-H3": (4, 4, 3),
    "5x4-H3": (5, 4, 3),
    "7x7-H2": (7, 7, 2),
    "3x3-H12": (3, 3, 12),     # 364 gametes, 12 376 progeny genotypes
}
ROW_KINDS = ("random", "one-hot", "no-reads")


def unrank(index, k):
    """The ascending multiset of k haplotypes at VCF index `index`."""
    g, rem = [0] * k, int(index)
    for p in range(k, 0, -1):
        n = 0
        while comb(n + p, p) <= rem:
            n += 1
        rem -= comb(n + p - 1, p)
        g[p - 1] = n
    return g


def rank(g):
    """The VCF index of the ascending multiset g."""
    return sum(comb(int(x) + i, i + 1) for i, x in enumerate(g))


def log_evidence(gam_a, gam_b, llk_c, H, t_a, t_b):
    """float64 [n_a, n_b]: the definition in long double, rounded at the end.  A NaN likelihood, or none that is finite: NaN."""
    A = np.atleast_2d(np.asarray(gam_a, dtype=np.float64)).astype(LD)
    B = np.atleast_2d(np.asarray(gam_b, dtype=np.float64)).astype(LD)
    llk = np.asarray(llk_c, dtype=np.float64).astype(LD)
    if np.any(np.isnan(llk)) or not np.any(np.isfinite(llk)):
        return np.full((len(A), len(B)), np.nan)
    z = np.zeros((len(A), len(B)), dtype=LD)
    gb = [unrank(b, t_b) for b in range(B.shape[1])]
    for a in range(A.shape[1]):
        ga = unrank(a, t_a)
        for b in range(B.shape[1]):
            t = np.exp(llk[rank(sorted(ga + gb[b]))])
            if t != 0:
                z += t * (A[:, a, None] * B[None, :, b])
    with np.errstate(divide="ignore"):
        return np.log(z).astype(np.float64)


def draw_rows(rng, H, t, f, kinds):
    """float64 [len(kinds), NA]: gamete rows.  The first three are those of parents of ploidy 2t (application.gamete_table):
    `random` a drawn posterior at a gamete error of 0.01, `one-hot` one genotype at an error of 0 -- most gametes exactly 0 --,
    `no-reads` the flat posterior.  The rows after them are drawn over the gametes themselves, which costs no walk over the
    parent's genotypes: a drawn distribution, a single gamete, the population's row."""
    G, NA = comb(H + 2 * t - 1, 2 * t), comb(H + t - 1, t)
    rows = []
    for i, kind in enumerate(kinds):
        if i >= 3:
            one = np.zeros(NA)
            one[rng.integers(NA)] = 1.0
            rows.append({"random": rng.dirichlet(np.full(NA, 0.5)), "one-hot": one}.get(kind, application.population_gametes(H, t, f)))
        elif kind == "random":
            rows.append(application.gamete_table(rng.dirichlet(np.full(G, 0.5)), H, 2 * t, f, 0.01))
        elif kind == "one-hot":
            p = np.zeros(G)
            p[rng.integers(G)] = 1.0
            rows.append(application.gamete_table(p, H, 2 * t, f, 0.0))
        else:
            rows.append(application.gamete_table(np.full(G, 1.0 / G), H, 2 * t, f, 0.01))
    return np.stack(rows)


def draw_case(name, n=3, n_progeny=3, records=1):
    """The drawn inputs of a shape: (t_a, t_b, H, gam_a [records, n, NA], gam_b [records, n, NB], llk [records, n_progeny, G_c],
    f [records, H]).  The rows cycle through ROW_KINDS; record 0 has a zero frequency; the progeny's likelihoods are drawn, the
    second progeny's with all but a few genotypes impossible."""
    t_a, t_b, H = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(("parentage-%s-%d-%d-%d" % (name, n, n_progeny, records)).encode()))
    GC = comb(H + t_a + t_b - 1, t_a + t_b)
    fr = rng.dirichlet(np.full(H, 2.0), size=records)
    fr[0, 1 % H] = 0.0
    fr[0] /= fr[0].sum()
    kinds = [ROW_KINDS[i % len(ROW_KINDS)] for i in range(n)]
    gam_a = np.stack([draw_rows(rng, H, t_a, fr[r], kinds) for r in range(records)])
    gam_b = np.stack([draw_rows(rng, H, t_b, fr[r], kinds[::-1]) for r in range(records)])
    llk = -rng.exponential(4.0, size=(records, n_progeny, GC))
    if n_progeny > 1:
        llk[:, 1, rng.random(GC) < 0.7] = -np.inf
        llk[:, 1, 0] = -2.0
    return t_a, t_b, H, gam_a, gam_b, llk, fr


def within(got, want, floor=FLOOR):
    """(every entry within REL |want| + floor -- equal NaNs agree, -inf must be -inf --, the largest |got - want| of the finite)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or np.any(np.isnan(got) != np.isnan(want)) or np.any(np.isinf(got) != np.isinf(want)):
        return False, np.inf
    if np.any(got[np.isinf(want)] != want[np.isinf(want)]):
        return False, np.inf
    live = np.isfinite(want)
    err = np.abs(got[live] - want[live])
    return bool(np.all(err <= REL * np.abs(want[live]) + floor)), float(err.max()) if err.size else 0.0
