"""The float64 host definition of the cross prior -- application.gamete_table, cross_prior_tables, cross_prior_unit -- against what
the reference gives (tests/golden/cross_prior.npz: gamete_probabilities / cross_probabilities on drawn parent posteriors, and
exp(trio_log_pmf) with lambda = 0 for one-hot parents; tests/golden/make_cross_prior.py) and against the long-double restatement
in plain loops (tests/cross_reference.py), whose ENVELOPE the GPU tests' bound rests on.  CPU only."""
import os
import zlib
from math import comb

import numpy as np
import pytest

from mchap_amd import application
from tests import cross_reference as ref

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_prior.npz")
# the reference works in float64 too (sums of products in another order; part 2 through logarithms): a few roundings of values <= 1
FIXTURE_ATOL = 1e-14


@pytest.fixture(scope="module")
def fixture():
    z = np.load(FIXTURE)
    return z, [str(n) for n in z["names"]]


def test_the_fixture_holds_what_the_issue_lists(fixture):
    z, names = fixture
    assert sum(n.startswith("part1_") for n in names) == 9 and sum(n.startswith("part2_") for n in names) == 54
    assert {tuple(z[n + "_shape"][1:]) for n in names if n.startswith("part2_")} == {(4, 2), (6, 4), (8, 8)}
    assert np.any(z["part2_freqs"] == 0.0)


def test_gametes_and_cross_of_drawn_parents(fixture):
    z, names = fixture
    for name in (n for n in names if n.startswith("part1_")):
        H, KP, KQ = (int(x) for x in z[name + "_shape"])
        gam_p, gam_q, X = application.cross_prior_tables(z[name + "_pp"], KP, z[name + "_pq"], KQ, H)
        for got, key in ((gam_p, "_gam_p"), (gam_q, "_gam_q"), (X, "_x")):
            want = z[name + key]
            np.testing.assert_allclose(got, want, rtol=0, atol=FIXTURE_ATOL, err_msg=name + key)
            assert np.array_equal(got == 0.0, want == 0.0), name + key
            assert abs(got.sum() - 1.0) <= 1e-12
        # the same through the unit's form: the posterior itself as the likelihood under the flat genotype prior
        with np.errstate(divide="ignore"):
            unit = application.cross_prior_unit(np.log(z[name + "_pp"]), KP, None, np.log(z[name + "_pq"]), KQ, None, H, None, (0.0, 0.0))
        np.testing.assert_allclose(unit["X"], z[name + "_x"], rtol=0, atol=FIXTURE_ATOL)
        assert np.array_equal(unit["X"] == 0.0, z[name + "_x"] == 0.0) and np.array_equal(unit["log_x"] == -np.inf, unit["X"] == 0.0)


def test_the_trio_pmf_of_one_hot_parents(fixture):
    z, names = fixture
    freqs = z["part2_freqs"]
    zeros = 0
    for name in (n for n in names if n.startswith("part2_")):
        H, KP, KQ = (int(x) for x in z[name + "_shape"])
        fi, ep, eq, ip, iq = z[name + "_case"]
        llk_p, llk_q = np.full(comb(H + KP - 1, KP), -np.inf), np.full(comb(H + KQ - 1, KQ), -np.inf)
        llk_p[int(ip)] = llk_q[int(iq)] = 0.0
        unit = application.cross_prior_unit(llk_p, KP, None, llk_q, KQ, None, H, freqs[int(fi)], (float(ep), float(eq)))
        want = z[name + "_x"]
        np.testing.assert_allclose(unit["X"], want, rtol=0, atol=FIXTURE_ATOL, err_msg=name)
        assert np.array_equal(unit["X"] == 0.0, want == 0.0), name          # exactly 0 where the reference's is
        assert abs(unit["X"].sum() - 1.0) <= 1e-12
        zeros += int(np.sum(want == 0.0))
    assert zeros > 100


def trio_inputs(name, kind, prior, error):
    """The drawn inputs of a case: (K_P, K_Q, H, llk_p, llk_q, llk_c, F, f)."""
    KP, KQ, H = ref.CASES[name]
    rng = np.random.default_rng(zlib.crc32(("cross-%s-%s-%s-%g" % (name, kind, prior, error)).encode()))
    llk_p = ref.parent_llk(rng, kind, comb(H + KP - 1, KP))
    llk_q = ref.parent_llk(rng, "random" if kind == "no-reads" else kind, comb(H + KQ - 1, KQ))
    llk_c = -rng.exponential(4.0, size=comb(H + KP // 2 + KQ // 2 - 1, KP // 2 + KQ // 2))
    fr = ref.draw_frequencies(rng, H)
    F, f = {"flat": (None, fr[1]), "F0-zero-frequency": (0.0, fr[0]), "F-positive": (ref.F_POSITIVE, fr[1])}[prior]
    return KP, KQ, H, llk_p, llk_q, llk_c, F, f


def test_the_host_definition_stays_within_the_envelope():
    worst, at = 0.0, None
    for name in ref.CASES:
        for kind in ref.PARENT_KINDS:
            for prior in ("flat", "F0-zero-frequency", "F-positive"):
                for error in (0.0, 0.01):
                    KP, KQ, H, llk_p, llk_q, llk_c, F, f = trio_inputs(name, kind, prior, error)
                    got = application.cross_prior_unit(llk_p, KP, F, llk_q, KQ, F, H, f, (error, error), llk_c)
                    want = ref.trio(llk_p, KP, F, llk_q, KQ, F, H, f, (error, error), llk_c)
                    for key in ("gam_p", "gam_q", "X", "q"):
                        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), (name, kind, prior, error, key)
                        assert np.array_equal(got[key] == 0.0, want[key] == 0.0), (name, kind, prior, error, key)
                        live = ~np.isnan(want[key])
                        err = float(np.max(np.abs(got[key][live] - want[key][live]))) if live.any() else 0.0
                        if err > worst:
                            worst, at = err, (name, kind, prior, error, key)
                    if not np.any(np.isnan(want["X"])):
                        assert abs(got["X"].sum() - 1.0) <= 1e-12
                        assert got["mode"] == int(np.argmax(got["q"])) and got["mode_prob"] == pytest.approx(got["q"].max(), rel=1e-12)
    print("largest |float64 - long double| of a probability: %.3g at %r (ENVELOPE %g at %s)" % (worst, at, ref.ENVELOPE, ref.ENVELOPE_CASE))
    assert worst <= ref.ENVELOPE
