"""The float64 host definition of the parentage evidence -- application.parentage_unit -- against the long-double restatement in
plain loops (tests/parentage_reference.py), whose ENVELOPE the GPU tests' bound rests on; against the cross evidence of
application.cross_prior_unit, which goes through the cross prior X; and against X as the reference gives it
(tests/golden/cross_prior.npz).  CPU only."""
import os
import zlib
from math import comb

import numpy as np
import pytest

from mchap_amd import application
from tests import parentage_reference as ref

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_prior.npz")


@pytest.fixture(scope="module")
def cases():
    return {name: ref.draw_case(name) for name in ref.SHAPES}


def test_the_host_definition_stays_within_the_envelope(cases):
    worst, at = 0.0, None
    for name, (t_a, t_b, H, gam_a, gam_b, llk, _) in cases.items():
        for c in range(llk.shape[1]):
            got = application.parentage_unit(gam_a[0], gam_b[0], llk[0, c], H, t_a, t_b)
            want = ref.log_evidence(gam_a[0], gam_b[0], llk[0, c], H, t_a, t_b)
            ok, err = ref.within(got, want)
            assert ok, (name, c, err)
            if err > worst:
                worst, at = err, (name, c)
    print("largest |float64 - long double| of a log evidence: %.3g at %r (ENVELOPE %g at %s)" % (worst, at, ref.ENVELOPE, ref.ENVELOPE_CASE))
    assert worst <= ref.ENVELOPE


def test_the_edges_of_the_definition(cases):
    t_a, t_b, H, gam_a, gam_b, llk, _ = cases["2x2-H3"]
    A, B = gam_a[0], gam_b[0]
    # a progeny without reads: exactly 0
    assert np.array_equal(application.parentage_unit(A, B, None, H, t_a, t_b), np.zeros((3, 3)))
    # a NaN row: its row or column, and nothing else
    full = application.parentage_unit(A, B, llk[0, 0], H, t_a, t_b)
    An = A.copy()
    An[1] = np.nan
    got = application.parentage_unit(An, B, llk[0, 0], H, t_a, t_b)
    assert np.all(np.isnan(got[1])) and np.array_equal(got[[0, 2]], full[[0, 2]])
    Bn = B.copy()
    Bn[1] = np.nan
    got = application.parentage_unit(A, Bn, llk[0, 0], H, t_a, t_b)
    assert np.all(np.isnan(got[:, 1])) and np.array_equal(got[:, [0, 2]], full[:, [0, 2]])
    # a NaN likelihood, or none that is finite: NaN throughout
    bad = llk[0, 0].copy()
    bad[3] = np.nan
    assert np.all(np.isnan(application.parentage_unit(A, B, bad, H, t_a, t_b)))
    assert np.all(np.isnan(application.parentage_unit(A, B, np.full(len(bad), -np.inf), H, t_a, t_b)))
    # one-hot parents at a gamete error of 0 that cannot make the progeny: exactly -inf
    G = comb(H + 3, 4)
    p0, p2 = np.zeros(G), np.zeros(G)
    p0[0], p2[G - 1] = 1.0, 1.0                      # 0/0/0/0 and 2/2/2/2
    f = np.full(H, 1.0 / H)
    rows = np.stack([application.gamete_table(p, H, 4, f, 0.0) for p in (p0, p2)])
    only = np.full(comb(H + 3, 4), -np.inf)
    only[application._multiset_ranks(np.array([[1, 1, 1, 1]]))[0]] = -1.0
    assert np.all(application.parentage_unit(rows, rows, only, H, 2, 2) == -np.inf)


def test_every_pair_is_the_cross_evidence_through_the_cross_prior(cases):
    """parentage_unit sums over the pairs of gametes, cross_prior_unit over the progeny genotypes with X: the same number."""
    for name, (t_a, t_b, H, _, _, llk, fr) in cases.items():
        rng = np.random.default_rng(zlib.crc32(("parentage-cross-%s" % name).encode()))
        KP, KQ = 2 * t_a, 2 * t_b
        post = {K: [rng.dirichlet(np.full(comb(H + K - 1, K), 0.5)) for _ in range(2)] for K in {KP, KQ}}
        for pp in post[KP]:
            for pq in post[KQ]:
                with np.errstate(divide="ignore"):
                    unit = application.cross_prior_unit(np.log(pp), KP, None, np.log(pq), KQ, None, H, fr[0], (0.01, 0.01), llk[0, 0])
                got = application.parentage_unit(unit["gam_p"], unit["gam_q"], llk[0, 0], H, t_a, t_b)
                ok, err = ref.within(got, np.array([[unit["log_z"]]]))
                assert ok, (name, err, got, unit["log_z"])


def test_a_case_of_the_reference_fixture():
    """The reference's own X (cross_probabilities on drawn parent posteriors): log sum_gc X[gc] exp(llk[gc]) from the fixture's
    array, the parents' posteriors through gamete_table."""
    z = np.load(FIXTURE)
    names = [str(n) for n in z["names"] if str(n).startswith("part1_")]
    assert names
    for name in names:
        H, KP, KQ = (int(x) for x in z[name + "_shape"])
        f = np.full(H, 1.0 / H)
        rng = np.random.default_rng(zlib.crc32(("parentage-fixture-%s" % name).encode()))
        llk = -rng.exponential(4.0, size=len(z[name + "_x"]))
        rows_p = application.gamete_table(z[name + "_pp"], H, KP, f, 0.0)[None]
        rows_q = application.gamete_table(z[name + "_pq"], H, KQ, f, 0.0)[None]
        got = application.parentage_unit(rows_p, rows_q, llk, H, KP // 2, KQ // 2)
        m = llk.max()
        want = m + np.log(np.sum(z[name + "_x"].astype(ref.LD) * np.exp((llk - m).astype(ref.LD))))
        # (X of the fixture is float64 of the reference: each entry within a few roundings, as tests/test_cross_prior_reference.py holds it)
        assert abs(got[0, 0] - float(want)) <= 1e-9 * abs(float(want)) + 1e-13, (name, got[0, 0], float(want))
