"""The float64 host definition of the family call -- application.family_unit, the factorised form that ships and that the GPU is
compared with -- against the unfactorised long-double restatement (tests/family_reference.py), whose ENVELOPE the GPU tests' bound
rests on, and the properties the definition has by construction.  CPU only."""
import functools
import zlib
from math import comb

import numpy as np
import pytest

from mchap_amd import application
from tests import cross_reference as cref
from tests import family_reference as ref

PRIORS = ("flat", "F0", "F-positive")
ERRORS = ((0.0, 0.0), (0.01, 0.05))
N_PROGENY = (0, 1, 4)
PRED_TOL = 1e-11   # of a predictive log evidence: a difference of two logarithms of sums the envelope bounds relatively


def family_inputs(name, kind, prior, errors, n):
    """The drawn inputs of a case: (K_P, K_Q, H, llk_p, llk_q, F, f, progeny) -- with n = 4 the third progeny has no reads."""
    KP, KQ, H = ref.CASES[name]
    rng = np.random.default_rng(zlib.crc32(("family-%s-%s-%s-%g-%d" % (name, kind, prior, errors[1], n)).encode()))
    llk_p = cref.parent_llk(rng, kind, comb(H + KP - 1, KP))
    llk_q = cref.parent_llk(rng, "random" if kind == "no-reads" else kind, comb(H + KQ - 1, KQ))
    GC = comb(H + KP // 2 + KQ // 2 - 1, KP // 2 + KQ // 2)
    progeny = [None if (n == 4 and c == 2) else -rng.exponential(4.0, size=GC) for c in range(n)]
    fr = cref.draw_frequencies(rng, H)
    F, f = {"flat": (None, fr[1]), "F0": (0.0, fr[1]), "F-positive": (cref.F_POSITIVE, fr[1])}[prior]
    return KP, KQ, H, llk_p, llk_q, F, f, progeny


@functools.lru_cache(maxsize=None)
def transmission(name, prior, errors):
    """X of a shape at the frequencies and gamete errors of a case (the draw of fr does not depend on kind or n: see below)."""
    KP, KQ, H, _, _, _, f, _ = family_inputs(name, "random", prior, errors, 0)
    return f, ref.transmission(ref.gamma_rows(H, KP, f, errors[0]), ref.gamma_rows(H, KQ, f, errors[1]), H, KP // 2, KQ // 2)


def test_the_host_definition_stays_within_the_envelope():
    worst, at = 0.0, None
    for name in ref.CASES:
        for kind in cref.PARENT_KINDS:
            for prior in PRIORS:
                for errors in ERRORS:
                    for n in N_PROGENY:
                        KP, KQ, H, llk_p, llk_q, F, _, progeny = family_inputs(name, kind, prior, errors, n)
                        f, X = transmission(name, prior, errors)
                        got = application.family_unit(llk_p, KP, F, llk_q, KQ, F, H, f, errors, progeny)
                        want = ref.family(llk_p, KP, F, llk_q, KQ, F, H, f, errors, progeny, X=X)
                        case = (name, kind, prior, errors, n)
                        pairs = [(got["post_p"], want["post_p"], "post_p"), (got["post_q"], want["post_q"], "post_q")]
                        pairs += [(g, w, "q%d" % c) for c, (g, w) in enumerate(zip(got["q"], want["q"]))]
                        for g, w, key in pairs:
                            assert np.array_equal(np.isnan(g), np.isnan(w)), case + (key,)
                            assert np.array_equal(g == 0.0, w == 0.0), case + (key,)
                            live = ~np.isnan(w)
                            err = float(np.max(np.abs(g[live] - w[live]))) if live.any() else 0.0
                            if err > worst:
                                worst, at = err, case + (key,)
                            if live.all():
                                assert abs(g.sum() - 1.0) <= 1e-12, case + (key,)
                        assert np.array_equal(np.isnan(got["pred"]), np.isnan(want["pred"])), case
                        live = ~np.isnan(want["pred"])
                        assert np.all(np.abs(got["pred"][live] - want["pred"][live]) <= PRED_TOL * np.maximum(1.0, np.abs(want["pred"][live]))), case
                        if n == 4 and live.all():
                            assert got["pred"][2] == 0.0
    print("largest |float64 - long double| of a probability: %.3g at %r (ENVELOPE %g at %s)" % (worst, at, ref.ENVELOPE, ref.ENVELOPE_CASE))
    assert worst <= ref.ENVELOPE


def drawn(name="4x4-H3", seed=3, n=3, kind="random"):
    KP, KQ, H = ref.CASES[name]
    rng = np.random.default_rng(seed)
    llk_p = cref.parent_llk(rng, kind, comb(H + KP - 1, KP))
    llk_q = cref.parent_llk(rng, kind, comb(H + KQ - 1, KQ))
    GC = comb(H + KP // 2 + KQ // 2 - 1, KP // 2 + KQ // 2)
    return KP, KQ, H, llk_p, llk_q, cref.draw_frequencies(rng, H)[1], [-rng.exponential(4.0, size=GC) for _ in range(n)]


@pytest.mark.parametrize("name", ["4x4-H3", "4x2-H4", "6x6-H3"])
def test_without_progeny_the_parents_own_posteriors(name):
    KP, KQ, H, llk_p, llk_q, f, _ = drawn(name)
    for F in (None, 0.3):
        got = application.family_unit(llk_p, KP, F, llk_q, KQ, 0.0, H, f, (0.01, 0.05), [])
        np.testing.assert_allclose(got["post_p"], application._unit_posterior(llk_p, H, KP, F, f)[0], rtol=0, atol=1e-14)
        np.testing.assert_allclose(got["post_q"], application._unit_posterior(llk_q, H, KQ, 0.0, f)[0], rtol=0, atol=1e-14)
        assert len(got["q"]) == 0 and len(got["pred"]) == 0
        norm = application._unit_posterior(llk_p, H, KP, F, f)[1] + application._unit_posterior(llk_q, H, KQ, 0.0, f)[1]
        assert got["log_z"] == pytest.approx(norm, abs=1e-12)


def test_progeny_without_reads_change_no_bit_of_the_parents():
    KP, KQ, H, llk_p, llk_q, f, progeny = drawn()
    base = application.family_unit(llk_p, KP, 0.3, llk_q, KQ, 0.3, H, f, (0.01, 0.05), progeny)
    more = application.family_unit(llk_p, KP, 0.3, llk_q, KQ, 0.3, H, f, (0.01, 0.05), [None, progeny[0], None, progeny[1], progeny[2], None])
    assert base["post_p"].tobytes() == more["post_p"].tobytes() and base["post_q"].tobytes() == more["post_q"].tobytes()
    assert base["log_z"] == more["log_z"]
    for c, at in enumerate((1, 3, 4)):
        assert base["q"][c].tobytes() == more["q"][at].tobytes() and base["pred"][c] == more["pred"][at]
    for at in (0, 2, 5):
        assert more["pred"][at] == 0.0 and abs(more["q"][at].sum() - 1.0) <= 1e-12
        assert more["q"][at].tobytes() == more["q"][0].tobytes()


def test_swapping_the_parents_swaps_the_outputs():
    KP, KQ, H, llk_p, llk_q, f, progeny = drawn("4x2-H4")
    one = application.family_unit(llk_p, KP, 0.3, llk_q, KQ, None, H, f, (0.01, 0.05), progeny)
    two = application.family_unit(llk_q, KQ, None, llk_p, KP, 0.3, H, f, (0.05, 0.01), progeny)
    np.testing.assert_allclose(one["post_p"], two["post_q"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(one["post_q"], two["post_p"], rtol=1e-12, atol=1e-15)
    for a, b in zip(one["q"], two["q"]):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(one["pred"], two["pred"], rtol=0, atol=1e-12)
    assert one["log_z"] == pytest.approx(two["log_z"], abs=1e-12)


@pytest.mark.parametrize("name", ["4x4-H3", "4x2-H4"])
def test_one_hot_parents_and_one_progeny_give_the_cross_posterior(name):
    KP, KQ, H, llk_p, llk_q, f, progeny = drawn(name, kind="one-hot", n=1)
    for errors in ERRORS:
        got = application.family_unit(llk_p, KP, None, llk_q, KQ, None, H, f, errors, progeny)
        want = application.cross_prior_unit(llk_p, KP, None, llk_q, KQ, None, H, f, errors, progeny[0])
        ok, err = cref.within(got["q"][0], want["q"])
        assert ok, (name, errors, err)
        assert got["modes"][0] == want["mode"]
        # the parents are known: the progeny's predictive evidence is the cross evidence
        assert got["pred"][0] == pytest.approx(want["log_z"], abs=1e-12)


def test_ten_progeny_move_a_parent_without_reads_to_their_haplotype():
    KP, KQ, H = 4, 4, 3
    f = np.array([0.6, 0.38, 0.02])                        # haplotype 2 is unlikely under the prior
    G = comb(H + 3, 4)
    table = application._genotype_table(H, 4)
    alone = application.family_unit(np.zeros(G), KP, 0.0, np.zeros(G), KQ, 0.0, H, f, (0.01, 0.01), [])
    assert 2 not in table[alone["mode_p"]] and 2 not in table[alone["mode_q"]]
    llk = np.where(np.sum(table == 2, axis=1) >= 1, -1.0, -40.0)   # every progeny carries haplotype 2
    got = application.family_unit(np.zeros(G), KP, 0.0, np.zeros(G), KQ, 0.0, H, f, (0.01, 0.01), [llk] * 10)
    assert 2 in table[got["mode_p"]] and 2 in table[got["mode_q"]]
    carries = np.sum(table == 2, axis=1) >= 1
    assert got["post_p"][carries].sum() > 0.5 > alone["post_p"][carries].sum()
    # ... and with the other parent known not to carry it, P's mode has it
    llk_q = np.where(carries, -np.inf, 0.0)
    got = application.family_unit(np.zeros(G), KP, 0.0, llk_q, KQ, 0.0, H, f, (0.01, 0.01), [llk] * 10)
    assert 2 in table[got["mode_p"]] and got["post_p"][carries].sum() > 1.0 - 1e-9


def test_the_predictive_evidence_is_the_difference_of_two_family_evidences():
    for name, errors in (("4x4-H3", (0.01, 0.05)), ("4x2-H4", (0.0, 0.0)), ("6x6-H3", (0.01, 0.05))):
        KP, KQ, H, llk_p, llk_q, f, progeny = drawn(name, n=4)
        progeny[1] = None
        full = application.family_unit(llk_p, KP, 0.3, llk_q, KQ, 0.0, H, f, errors, progeny)
        for c in range(4):
            less = application.family_unit(llk_p, KP, 0.3, llk_q, KQ, 0.0, H, f, errors, progeny[:c] + progeny[c + 1:])
            assert full["pred"][c] == pytest.approx(full["log_z"] - less["log_z"], abs=1e-11), (name, c)


def test_the_null_record():
    KP, KQ, H, llk_p, llk_q, f, progeny = drawn()
    dead = np.full(len(llk_p), -np.inf)
    for got in (application.family_unit(dead, KP, 0.3, llk_q, KQ, 0.3, H, f, (0.01, 0.01), progeny),
                application.family_unit(llk_p, KP, 0.3, llk_q, KQ, 0.3, H, f, (0.01, 0.01), [progeny[0], np.full(len(progeny[0]), -np.inf)])):
        assert np.all(np.isnan(got["post_p"])) and np.all(np.isnan(got["post_q"])) and np.isnan(got["log_z"])
        assert got["mode_p"] == -1 and got["mode_q"] == -1 and np.all(got["modes"] == -1) and np.all(np.isnan(got["pred"]))
        assert all(np.all(np.isnan(x)) for x in got["q"])
    # Z = 0: one-hot parents, no gamete error, a progeny they cannot have
    table = application._genotype_table(H, 4)
    one = lambda g: np.where(np.all(table == np.array(g), axis=1), 0.0, -np.inf)   # noqa: E731
    got = application.family_unit(one([0, 0, 0, 0]), KP, None, one([0, 0, 1, 1]), KQ, None, H, f, (0.0, 0.0), [one([2, 2, 2, 2])])
    assert np.isnan(got["log_z"]) or got["log_z"] == -np.inf
    assert got["mode_p"] == -1 and np.all(np.isnan(got["q"][0]))
