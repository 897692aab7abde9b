"""The long-double reference of one iteration of the frequency estimate (tests/estimate_reference.py), anchored: its genotype
table against calling.index_as_genotype_alleles, its frequencies against the brute force of tests/estimate_units.py and against
the oracle-backed definition, and -- the condition that fixes the range of F the GPU cases use -- against the kernels' own lgamma
form in float64 on every input of tests/test_gpu_estimate_kernels.py.  CPU only."""
from math import comb

import numpy as np
import pytest

from mchap_amd import application, calling
from tests import estimate_cases as cases
from tests import estimate_reference as ref
from tests.estimate_units import brute_sample_frequencies, fresh, make_record, per_sample, samples_of
from tests.test_estimate_frequencies import SHAPES

# what two float64 evaluations of the iteration may differ by: 1e-11 relative with an absolute floor of 1e-12
REL, FLOOR = 1e-11, 1e-12

TABLE_SHAPES = sorted({(K, H) for K, H, _ in cases.CASES.values()} | {(K, H) for H in cases.LAYOUT_HAPS for K in (2, 4)} |
                      {(2, 2), (3, 4), (6, 12), (1, 1)})


@pytest.mark.parametrize("K,H", TABLE_SHAPES)
def test_genotype_table_is_vcf_order(K, H):
    g = ref.genotype_table(H, K)
    G = comb(H + K - 1, K)
    assert g.shape == (G, K) and g.dtype == np.int64
    assert np.all(np.diff(g, axis=1) >= 0) and g.min() >= 0 and g.max() == H - 1
    if G <= 5000:
        idx = np.arange(G)
    else:
        idx = np.unique(np.concatenate([np.arange(32), np.arange(G - 32, G), np.random.default_rng(K * 1000 + H).integers(0, G, size=2000)]))
    for i in idx:
        assert g[i].tolist() == calling.index_as_genotype_alleles(int(i), K).tolist(), i


def _llk64(sr, haps, K):
    """float64 log likelihoods of one sample's reads over genotype_table(H, K): log of the mean over the genotype's haplotypes of
    the product of a read's probabilities (a gap counts 1), weighted by the read's count."""
    dists, counts = sr["dists"], sr["counts"]
    g = ref.genotype_table(len(haps), K)
    llk = np.zeros(len(g))
    for r in range(len(dists)):
        p = np.ones(len(haps))
        for j in range(dists.shape[1]):
            v = dists[r, j, haps[:, j]]
            p *= np.where(np.isnan(v), 1.0, v)
        llk += counts[r] * np.log(p[g].sum(axis=1) / K)
    return llk


def _record(name):
    H, M, ploidies, n_reads, inbreeding, masked = SHAPES[name]
    unit = make_record(np.random.default_rng(11 + len(name)), H, M, ploidies, n_reads, masked=masked)
    haps = unit["locus"].haplotypes
    rec = dict(H=H, f=np.array(unit["locus"].frequencies),
               units=[(_llk64(unit["reads"]["S%d" % s], haps, ploidies[s]), ploidies[s], inbreeding[s]) for s in range(len(ploidies))])
    return unit, rec


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_reference_against_brute_force(name):
    H, M, ploidies, n_reads, inbreeding, masked = SHAPES[name]
    unit, rec = _record(name)
    haps, f = unit["locus"].haplotypes, rec["f"]
    acc = np.zeros(H)
    for s, (llk, K, F) in enumerate(rec["units"]):
        sr = unit["reads"]["S%d" % s]
        want = brute_sample_frequencies(sr["dists"], sr["counts"], haps, K, F, f)
        got = (ref.unit_allele_counts(llk, ref.genotype_table(H, K), H, K, F, f) / K).astype(np.float64)
        ok, dev = ref.deviation(got, want, REL, FLOOR)
        print(name, "sample", s, "reference vs brute force: %.3g relative" % dev)
        assert ok, (got, want)
        acc += K * want
    ok, dev = ref.deviation(ref.iterate([rec])[0], acc / sum(ploidies), REL, FLOOR)
    print(name, "iteration, reference vs brute force: %.3g relative" % dev)
    assert ok
    if masked:
        assert ref.iterate([rec])[0][0] == 0.0


@pytest.mark.parametrize("name", ["ploidies_2_and_4", "refmasked"])
def test_the_reference_against_the_oracle_backed_definition(name):
    from tests.replay_call_exact import OracleBackend

    H, M, ploidies, n_reads, inbreeding, masked = SHAPES[name]
    unit, rec = _record(name)
    units = fresh([unit])
    want, it = application.estimate_prior_frequencies(units, samples_of(units), per_sample(ploidies), per_sample(inbreeding), 1,
                                                      tolerance=0.0, backend=OracleBackend())[0]
    ok, dev = ref.deviation(ref.iterate([rec])[0], want, REL, FLOOR)
    print(name, "reference vs oracle-backed definition: %.3g relative" % dev)
    assert it == 1 and ok


def _envelope(records):
    want, got = ref.iterate(records), ref.iterate_lgamma(records)
    oks, devs = zip(*(ref.deviation(g, w, REL, FLOOR) for g, w in zip(got, want)))
    return all(oks), max(devs)


@pytest.mark.parametrize("name", list(cases.CASES) + ["layout"])
def test_the_lgamma_form_keeps_the_digits_on_every_gpu_case(name):
    """The kernels' form of the prior -- differences of lgamma at alpha = f (1 - F) / F -- in float64 with the host's lgamma, on the
    inputs of tests/test_gpu_estimate_kernels.py: within 1e-11 relative of the long-double reference, which is what lets those
    tests ask 1e-9 of the kernels for F = 0 and 1e-4 <= F <= 0.99."""
    records = cases.build_layout()[0] if name == "layout" else cases.build_case(name)
    for r in records:
        assert all(F in cases.F_VALUES for _, _, F in r["units"])
    ok, dev = _envelope(records)
    print(name, "lgamma form in float64 vs long double: %.3g relative" % dev)
    assert ok


def test_what_the_lgamma_form_loses_outside_the_envelope():
    """Per F, the worst deviation of the float64 lgamma form from the long-double reference over ploidies 1 to 15, uniform tables
    of scale 5, 50 and 400, with and without zero frequencies on the two highest alleles.  Inside the envelope it stays under
    1e-11; at F = 1e-6 (alpha about 1e6 f, lgamma(alpha) about 1e7 with an ulp of 2e-9) the formula itself loses the digits: printed,
    and the reason F = 1e-6 is not among the GPU cases."""
    worst = {}
    for F in (0.0, 1e-6, 1e-4, 1e-3, 0.1, 0.5, 0.99):
        rng = np.random.default_rng(7)
        w = 0.0
        for K, H in ((10, 7), (3, 29), (2, 91), (15, 6), (1, 5), (4, 17)):
            for scale in (5.0, 50.0, 400.0):
                for variant in ("no_zeros", "top_two_zero"):
                    f = cases.frequency_row(rng, H, variant)
                    rec = dict(H=H, f=f, units=[(-scale * rng.random(comb(H + K - 1, K)), K, F)])
                    ok, dev = _envelope([rec])
                    w = max(w, dev)
                    assert ok or F == 1e-6, (F, K, H, scale, variant, dev)
        worst[F] = w
        print("F = %g: lgamma form in float64 vs long double, worst %.3g relative" % (F, w))
