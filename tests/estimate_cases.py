"""The synthetic inputs of the tests of the frequency-estimate kernels (tests/test_gpu_estimate_kernels.py; the CPU test
tests/test_estimate_reference.py checks the envelope of F on the very same inputs; tests/fuzz_estimate.py draws from the same
kinds): likelihood tables and frequency rows by kind, built so that every unit keeps a finite genotype."""
import zlib
from math import comb

import numpy as np

from tests.estimate_reference import genotype_table

TILE = 4096                                    # genotypes of a workgroup (EXACT_GENOS_PER_BLOCK)
F_VALUES = (0.0, 1e-4, 0.1, 0.5, 0.99)         # F = 0 and the envelope 1e-4 <= F <= 0.99
TABLE_KINDS = ("uniform5", "uniform400", "uniform1e5", "peaked", "holes")
VARIANTS = ("no_zeros", "refmasked", "top_two_zero")

# name: (K, H, three chained steps)
CASES = {
    "haploid": (1, 5, False),
    "one-haplotype": (4, 1, False),
    "tile-less-one": (2, 90, False),
    "tail-of-90": (2, 91, False),
    "cut-run": (3, 29, True),
    "K4-H17": (4, 17, False),
    "last-of-KM8": (8, 8, False),
    "first-of-KM16": (9, 8, False),
    "K10-H7": (10, 7, True),
    "K15-H6": (15, 6, False),
    "lds-above-64K": (2, 500, False),
}


def em_lds_bytes(H, K):
    """exact_em_lds (exact_kernel.hpp), restated: the staging tile, the prior tables, the wavefronts' accumulators."""
    return (256 * 17 + H * (K + 1) + (K + 1) + H + (H + 1) * 4 + 8) * 8


def frequency_row(rng, H, variant):
    """A Dirichlet(2) draw over H alleles (no component so small that a product of 15 of them leaves float64), with the variant's
    zeros: none, the reference allele (REFMASKED), or the two highest alleles."""
    f = rng.dirichlet(np.full(H, 2.0))
    if variant == "refmasked":
        f[0] = 0.0
    elif variant == "top_two_zero":
        f[-2:] = 0.0
    else:
        assert variant == "no_zeros"
    assert f.sum() > 0
    return f / f.sum()


def variants_for(H):
    """The variants a row of H alleles can take and still leave an allele."""
    return VARIANTS if H >= 3 else (VARIANTS[:2] if H == 2 else VARIANTS[:1])


def prior_finite(H, K, f):
    """bool [G]: the genotypes without an allele of frequency 0."""
    return np.all(np.asarray(f)[genotype_table(H, K)] > 0, axis=1)


def likelihood_table(rng, H, K, kind, f):
    """float64 [G] of `kind`; `f` is the row the unit is first run with, so that a finite genotype can be kept:
    uniform*: uniform in [-s, 0]; peaked: one genotype of the last tile at 0, the others in [-2e4, -1e4); holes: uniform in [-5, 0]
    with a tenth of the entries -inf and the whole first tile -inf -- unless nothing finite under the prior lies beyond it."""
    G = comb(H + K - 1, K)
    fin = prior_finite(H, K, f)
    assert fin.any()
    if kind.startswith("uniform"):
        llk = -float(kind[7:]) * rng.random(G)
    elif kind == "peaked":
        llk = -1e4 - 1e4 * rng.random(G) - 1e-3
        llk[int(rng.integers((G - 1) // TILE * TILE, G))] = 0.0
    else:
        assert kind == "holes"
        llk = -5.0 * rng.random(G)
        llk[rng.random(G) < 0.1] = -np.inf
        if np.any(fin[TILE:] & np.isfinite(llk[TILE:])):
            llk[:TILE] = -np.inf
        elif not np.any(fin & np.isfinite(llk)):
            llk[int(np.flatnonzero(fin)[0])] = -1.0
    assert np.any(fin & np.isfinite(llk)), "a unit without a finite genotype"
    return llk


def draw_inbreeding(rng, n):
    """n values of F_VALUES with F = 0 and F > 0 both present (n >= 2)."""
    F = [0.0, float(rng.choice(F_VALUES[1:]))] + [float(rng.choice(F_VALUES)) for _ in range(n - 2)]
    return [F[i] for i in rng.permutation(n)]


LAYOUT_HAPS, LAYOUT_STRIDE, LAYOUT_SAMPLES = (3, 7, 29), 32, 70


def build_layout():
    """The layout case: three records of 3, 7 and 29 haplotypes over the same 70 samples of ploidy 2 or 4 (both occur), one
    frequency variant each; the units of a record in sample order.  -> (records, ploidies [70])."""
    rng = np.random.default_rng(zlib.crc32(b"layout"))
    ploidies = rng.choice([2, 4], size=LAYOUT_SAMPLES)
    ploidies[:2] = (2, 4)
    Fs = draw_inbreeding(rng, LAYOUT_SAMPLES)
    records = []
    for H, variant in zip(LAYOUT_HAPS, VARIANTS):
        f = frequency_row(rng, H, variant)
        kinds = [str(k) for k in rng.choice(TABLE_KINDS, size=LAYOUT_SAMPLES)]
        records.append(dict(H=H, f=f, variant=variant, kinds=kinds,
                            units=[(likelihood_table(rng, H, int(ploidies[s]), kinds[s], f), int(ploidies[s]), Fs[s])
                                   for s in range(LAYOUT_SAMPLES)]))
    return records, [int(k) for k in ploidies]


def build_case(name):
    """The records of a case: [dict(H, f, units [(llk, K, F)], variant, kinds)].  One record per frequency variant, three units
    each (F = 0 and F > 0 both among them), the table kinds dealt so that each occurs in the case; `lds-above-64K` is one record
    (the two highest alleles 0: the end of its last tile is -inf under the prior) with a unit of F = 0.1 and one of F = 0."""
    K, H, _ = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name == "lds-above-64K":
        f = frequency_row(rng, H, "top_two_zero")
        kinds = ["holes", "uniform400"]
        return [dict(H=H, f=f, variant="top_two_zero", kinds=kinds,
                     units=[(likelihood_table(rng, H, K, kinds[0], f), K, 0.1), (likelihood_table(rng, H, K, kinds[1], f), K, 0.0)])]
    variants = variants_for(H)
    n = 3 * len(variants)
    kinds = list(TABLE_KINDS) + [str(k) for k in rng.choice(TABLE_KINDS, size=max(0, n - len(TABLE_KINDS)))]
    kinds = [kinds[i] for i in rng.permutation(len(kinds))][:n]   # (every kind once where the case has five units or more)
    records = []
    for v, variant in enumerate(variants):
        f = frequency_row(rng, H, variant)
        Fs = draw_inbreeding(rng, 3)
        ks = [str(k) for k in kinds[3 * v:3 * v + 3]]
        records.append(dict(H=H, f=f, variant=variant, kinds=ks,
                            units=[(likelihood_table(rng, H, K, ks[u], f), K, Fs[u]) for u in range(3)]))
    return records
