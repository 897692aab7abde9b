"""The kernels of the cross calls -- exact_gamete_kernel<8|16>, exact_cross_prior_kernel<8|16>, exact_cross_post_kernel and its
combine, after the evidence launches for the normalisers -- driven through device.ExactCross on drawn likelihood tables, against
the float64 host definition (application.cross_prior_unit, cross_posterior; tests/test_cross_prior_reference.py holds it to the
reference's fixture and to long double on the CPU).  The bound, on probabilities: |got - want| <= 1e-9 |want| + 8 x ENVELOPE
(tests/cross_reference.py); exact zeros of the prior and -inf logarithms must match exactly.  Every launch holds 3 records x
(2 parents + 3 progeny): random parents under F = 0 with a zero frequency, one-hot parents, a parent without reads."""
import functools
import zlib
from math import comb

import numpy as np
import pytest

from tests import cross_reference as ref

pytestmark = pytest.mark.gpu

# name: (K_P, K_Q, H)
SHAPES = {
    "2x2-H2": (2, 2, 2),
    "2x2-H90-tile-less-one": (2, 2, 90),          # G_c = 4095
    "2x2-H91-tail": (2, 2, 91),                   # G_c = 4186
    "4x4-H3": (4, 4, 3),
    "4x4-H22-253-gametes": (4, 4, 22),
    "4x4-H23-276-gametes": (4, 4, 23),
    "4x2-H4-odd-progeny": (4, 2, 4),
    "8x8-H3-last-of-KM8": (8, 8, 3),
    "10x8-H3-first-of-KM16": (10, 8, 3),
    "14x14-H2": (14, 14, 2),
    "6x6-H16-several-tiles": (6, 6, 16),          # 54 264 genotypes
}
ERRORS = (0.0, 0.01)
CASES = [(n, e) for n in SHAPES for e in ERRORS if not (n.startswith("6x6") and e == 0.0)]   # (the large shape as one case)
FS, ROWS = [0.0, ref.F_POSITIVE, ref.F_POSITIVE], [0, 1, 2]
N_PROGENY = 3
LOG_TOL = 2e-9   # of a log evidence: a relative deviation REL of the evidence itself, and the rounding of the logarithm


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(freqs [3, H] -- row 0 with a zero --, llk_p [3][G_P], llk_q [3][G_Q], llk_c [3][3][G_c]): record 0 random parents, record 1
    one-hot parents, record 2 a parent without reads."""
    KP, KQ, H = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(("gpu-cross-%s" % name).encode()))
    GP, GQ, GC = comb(H + KP - 1, KP), comb(H + KQ - 1, KQ), comb(H + KP // 2 + KQ // 2 - 1, KP // 2 + KQ // 2)
    fr = ref.draw_frequencies(rng, H)
    llk_p = [ref.parent_llk(rng, kind, GP) for kind in ref.PARENT_KINDS]
    llk_q = [ref.parent_llk(rng, kind, GQ) for kind in ("random", "one-hot", "random")]
    llk_c = [[-rng.exponential(4.0, size=GC) for _ in range(N_PROGENY)] for _ in range(3)]
    return fr, llk_p, llk_q, llk_c


@functools.lru_cache(maxsize=None)
def host(name, error, flat=False):
    """The host definition of the three records: [(cross_prior_unit's dict, [(q, log_z, mode, mode_prob, log_norm)] per progeny)]."""
    from mchap_amd import application

    KP, KQ, H = SHAPES[name]
    fr, llk_p, llk_q, llk_c = inputs(name)
    out = []
    for r in range(3):
        F = None if flat else FS[r]
        unit = application.cross_prior_unit(llk_p[r], KP, F, llk_q[r], KQ, F, H, fr[r], (error, error))
        prog = []
        for llk in llk_c[r]:
            norm = application._unit_posterior(llk, H, KP // 2 + KQ // 2, F, fr[r])[1]
            prog.append(application.cross_posterior(llk, unit["log_x"]) + (norm,))
        out.append((unit, prog))
    return out


def device(name, error, order=(0, 1, 2), flat=False):
    """The three launches with the records' units in `order` -> (gam_p [3, .], gam_q, log_x [3, G_c], log_z [9], mode, mode_prob,
    log_norm, q [9, G_c]) on the host, in the order given."""
    import torch

    from mchap_amd.device import ExactCross

    KP, KQ, H = SHAPES[name]
    fr, llk_p, llk_q, llk_c = inputs(name)
    dev = ExactCross()
    up = lambda tables: torch.from_numpy(np.ascontiguousarray(np.concatenate(tables))).to(dev.device)  # noqa: E731
    order = list(order)
    Fs = None if flat else [FS[r] for r in order]
    rows = [ROWS[r] for r in order]
    gam_p = dev.gametes(up([llk_p[r] for r in order]), H, KP, Fs, rows, fr, error)
    gam_q = dev.gametes(up([llk_q[r] for r in order]), H, KQ, Fs, rows, fr, [error] * 3)
    log_x = dev.cross_prior(gam_p, gam_q, H, KP, KQ)
    # the progeny: record by record in `order`, each record's progeny in that direction too
    units = [(i, r, c) for i, r in enumerate(order) for c in (range(N_PROGENY) if order == [0, 1, 2] else reversed(range(N_PROGENY)))]
    got = dev.posteriors(up([llk_c[r][c] for _, r, c in units]), H, KP // 2 + KQ // 2, log_x, [i for i, _, _ in units],
                         None if flat else [FS[r] for _, r, _ in units], fr[[ROWS[r] for r in order]], full=True)
    torch.cuda.synchronize()
    assert dev.launches == 4
    return tuple(t.cpu().numpy() for t in (gam_p, gam_q, log_x) + got), [(r, c) for _, r, c in units]


def check(name, error, flat=False):
    want = host(name, error, flat)
    (gam_p, gam_q, log_x, log_z, mode, prob, log_norm, q), units = device(name, error, flat=flat)
    worst = 0.0
    for r in range(3):
        unit, _ = want[r]
        for got, key in ((gam_p[r], "gam_p"), (gam_q[r], "gam_q"), (np.exp(log_x[r]), "X")):
            ok, err = ref.within(got, unit[key])
            assert ok, (name, error, r, key, err)
            worst = max(worst, err)
        assert np.array_equal(log_x[r] == -np.inf, unit["X"] == 0.0)                     # exactly -inf where every product is 0
        assert abs(np.exp(log_x[r]).sum() - 1.0) <= 1e-9
    for u, (r, c) in enumerate(units):
        hq, hz, hmode, hprob, hnorm = want[r][1][c]
        ok, err = ref.within(q[u], hq)
        assert ok, (name, error, r, c, "q", err)
        worst = max(worst, err)
        assert abs(log_z[u] - hz) <= LOG_TOL * max(1.0, abs(hz)) and abs(log_norm[u] - hnorm) <= LOG_TOL * max(1.0, abs(hnorm))
        # the mode: the returned genotype's probability under the host definition lies within the bound of the host's maximum
        bound = ref.REL * hq.max() + ref.FLOOR
        assert 0 <= mode[u] < len(hq) and hq.max() - hq[mode[u]] <= bound and abs(prob[u] - hq.max()) <= bound
        assert prob[u] == q[u][mode[u]] or abs(prob[u] - q[u][mode[u]]) <= bound
        assert mode[u] == int(np.argmax(q[u]))                                           # the first maximum of the device's own q
    return worst


@pytest.mark.parametrize("name,error", CASES)
def test_the_three_launches_against_the_host_definition(name, error):
    worst = check(name, error)
    if error == 0.0:
        # random parents under a zero frequency, and one-hot parents: the prior has exact zeros
        assert any(np.any(unit["X"] == 0.0) for unit, _ in host(name, error))
    print("%s e=%g: worst |deviation| %.3g (REL %g, FLOOR %.3g)" % (name, error, worst, ref.REL, ref.FLOOR))


@pytest.mark.parametrize("name", ["4x4-H3", "4x2-H4-odd-progeny", "2x2-H91-tail"])
def test_the_flat_genotype_prior(name):
    check(name, 0.01, flat=True)


@pytest.mark.parametrize("name,error", [("4x4-H23-276-gametes", 0.01), ("2x2-H91-tail", 0.0), ("10x8-H3-first-of-KM16", 0.01)])
def test_reversed_units_give_equal_bits(name, error):
    base, units = device(name, error)
    again, _ = device(name, error)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(base, again))
    got, runits = device(name, error, order=(2, 1, 0))
    assert runits == units[::-1]
    for a, b in zip(base, got):
        assert a.tobytes() == b[::-1].tobytes()


def test_a_parent_without_a_finite_genotype_and_its_neighbours():
    import torch

    from mchap_amd.device import ExactCross

    name = "4x4-H3"
    KP, KQ, H = SHAPES[name]
    fr, llk_p, llk_q, llk_c = inputs(name)
    dev = ExactCross()
    up = lambda tables: torch.from_numpy(np.ascontiguousarray(np.concatenate(tables))).to(dev.device)  # noqa: E731
    dead = np.full(len(llk_p[1]), -np.inf)
    gam_p = dev.gametes(up([llk_p[0], dead, llk_p[2]]), H, KP, FS, ROWS, fr, 0.01)
    assert dev.log_norm.cpu().numpy()[1] == -np.inf
    gam_q = dev.gametes(up(llk_q), H, KQ, FS, ROWS, fr, 0.01)
    log_x = dev.cross_prior(gam_p, gam_q, H, KP, KQ)
    log_z, mode, prob, norm, q = dev.posteriors(up([llk_c[r][0] for r in range(3)]), H, 4, log_x, ROWS, FS, fr, full=True)
    gam_p, log_x, log_z, mode, prob, norm, q = (t.cpu().numpy() for t in (gam_p, log_x, log_z, mode, prob, norm, q))
    assert np.all(np.isnan(gam_p[1])) and np.all(np.isnan(log_x[1])) and np.isnan(log_z[1]) and mode[1] == -1 and np.isnan(prob[1])
    assert np.all(np.isnan(q[1])) and np.isfinite(norm[1])
    (bgp, _, blx, blz, bmode, bprob, _, bq), units = device(name, 0.01)
    for r in (0, 2):
        u = units.index((r, 0))
        assert gam_p[r].tobytes() == bgp[r].tobytes() and log_x[r].tobytes() == blx[r].tobytes()
        assert log_z[r] == blz[u] and mode[r] == bmode[u] and prob[r] == bprob[u] and q[r].tobytes() == bq[u].tobytes()
    # no progeny genotype with a finite term: log Z -inf, no mode
    none = np.full(len(llk_c[0][0]), -np.inf)
    log_z, mode, prob, _, q = dev.posteriors(up([none]), H, 4, torch.from_numpy(blx[:1].copy()).to(dev.device), [0], None, None, full=True)
    assert log_z.cpu().numpy()[0] == -np.inf and int(mode.cpu().numpy()[0]) == -1 and np.all(np.isnan(q.cpu().numpy()))


def test_refused_shapes_and_the_checks_on_the_host_copies():
    import torch

    from mchap_amd import _lib
    from mchap_amd.device import ExactCross

    L = _lib.lib()
    assert int(L.mchap_exact_gametes_workspace_bytes(1, 5, 16)) == -1 and int(L.mchap_exact_gametes_workspace_bytes(1, 1000, 14)) == -1
    assert int(L.mchap_exact_gametes_workspace_bytes(3, 5, 4)) > 0
    assert int(L.mchap_exact_cross_prior_workspace_bytes(1, 5, 3, 4)) == -1 and int(L.mchap_exact_cross_prior_workspace_bytes(1, 5, 4, 4)) == 0
    assert int(L.mchap_exact_cross_prior_workspace_bytes(1, 3000, 14, 14)) == -1
    assert int(L.mchap_exact_cross_posterior_workspace_bytes(1, 5, 16)) == -1 and int(L.mchap_exact_cross_posterior_workspace_bytes(2, 5, 4)) > 0
    dev = ExactCross()
    llk = torch.zeros(comb(3 + 4 - 1, 4), dtype=torch.float64, device=dev.device)
    fr = np.full((1, 3), 1.0 / 3)
    with pytest.raises(NotImplementedError):
        dev.gametes(llk, 3000, 14, None, [0], np.full((1, 3000), 1.0 / 3000), 0.0)
    with pytest.raises(ValueError, match="odd"):
        dev.gametes(torch.zeros(10, dtype=torch.float64, device=dev.device), 3, 3, None, [0], fr, 0.0)
    for bad in (1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            dev.gametes(llk, 3, 4, [bad], [0], fr, 0.0)
    for bad in (1.5, -1e-9, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            dev.gametes(llk, 3, 4, [0.1], [0], fr, bad)
    assert dev.launches == 0
    # e = 1: the gametes are the multinomial of the frequencies, whatever the parent
    f = np.array([[0.5, 0.3, 0.2]])
    got = dev.gametes(llk, 3, 4, None, [0], f, 1.0).cpu().numpy()[0]
    want = np.array([0.25, 0.3, 0.09, 0.2, 0.12, 0.04])
    assert ref.within(got, want)[0]


def test_a_fixture_case_and_the_calling_functions():
    import os

    from mchap_amd import application, calling

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_prior.npz"))
    name = "part1_4x4_H3"                      # (drawn posteriors with exact zeros)
    want = z[name + "_x"]
    got = calling.cross_genotype_prior(z[name + "_pp"], 4, z[name + "_pq"], 4, 3)
    assert np.all(np.abs(got - want) <= ref.REL * want + ref.FLOOR + 1e-14) and np.array_equal(got == 0.0, want == 0.0)
    part2 = [str(n) for n in z["names"] if str(n).startswith("part2_6x4_f1_e0.01_0.2")][0]
    fi, ep, eq, ip, iq = z[part2 + "_case"]
    pp, pq = np.zeros(comb(3 + 6 - 1, 6)), np.zeros(comb(3 + 4 - 1, 4))
    pp[int(ip)] = pq[int(iq)] = 1.0
    got = calling.cross_genotype_prior(pp, 6, pq, 4, 3, gamete_error=(ep, eq), frequencies=z["part2_freqs"][int(fi)])
    want = z[part2 + "_x"]
    assert np.all(np.abs(got - want) <= ref.REL * want + ref.FLOOR + 1e-14) and np.array_equal(got == 0.0, want == 0.0)
    rng = np.random.default_rng(5)
    llk = -rng.exponential(4.0, size=len(want))
    with np.errstate(divide="ignore"):
        post = calling.cross_genotype_posteriors(llk, np.log(got))
        hq = application.cross_posterior(llk, np.log(got))[0]
    assert ref.within(post, hq)[0] and abs(post.sum() - 1.0) <= 1e-9
