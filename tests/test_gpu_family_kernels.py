"""The kernels of the family calls (exact_family_kernel.hpp) driven through device.ExactFamily on drawn likelihood tables, against
the float64 host definition (application.family_unit; tests/test_family_reference.py holds it to the unfactorised long-double
restatement on the CPU).  The bound, on probabilities: tests/cross_reference.within's rule with the family's envelope,
|got - want| <= 1e-9 |want| + 8 x ENVELOPE (tests/family_reference.py); exact zeros and NaNs must match exactly.  Every launch holds
3 records x (2 parents + 4 progeny, the third without reads): random parents under F = 0, one-hot parents under F > 0, a parent
without reads under F > 0."""
import ctypes as C
import functools
import zlib
from math import comb

import numpy as np
import pytest

from tests import cross_reference as cref
from tests import family_reference as ref

pytestmark = pytest.mark.gpu

# name: (K_P, K_Q, H)
SHAPES = {
    "2x2-H2-one-lane": (2, 2, 2),
    "4x2-H4-unequal-parents": (4, 2, 4),
    "4x4-H6-126x126-pairs": (4, 4, 6),
    "6x6-H4-84x84-pairs": (6, 6, 4),
    "8x8-H3-last-of-KM8": (8, 8, 3),
    "10x8-H3-first-of-KM16": (10, 8, 3),
}
ERRORS = ((0.0, 0.0), (0.01, 0.05))
FS = [0.0, cref.F_POSITIVE, cref.F_POSITIVE]
N_PROGENY, NO_READS = 4, 2
LOG_TOL = 2e-9   # of a log evidence: a relative deviation REL of the evidence itself, and the rounding of the logarithm


def within(got, want):
    return cref.within(got, want, floor=ref.FLOOR)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(freqs [3, H], llk_p [3][G_P], llk_q [3][G_Q], llk_c [3][4][G_c], reads [3, 4])."""
    KP, KQ, H = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(("gpu-family-%s" % name).encode()))
    GP, GQ, GC = comb(H + KP - 1, KP), comb(H + KQ - 1, KQ), comb(H + KP // 2 + KQ // 2 - 1, KP // 2 + KQ // 2)
    fr = rng.dirichlet(np.full(H, 2.0), size=3)
    llk_p = [cref.parent_llk(rng, kind, GP) for kind in cref.PARENT_KINDS]
    llk_q = [cref.parent_llk(rng, kind, GQ) for kind in ("random", "one-hot", "random")]
    llk_c = [[-rng.exponential(4.0, size=GC) for _ in range(N_PROGENY)] for _ in range(3)]
    reads = np.ones((3, N_PROGENY), dtype=np.int32)
    reads[:, NO_READS] = 0
    return fr, llk_p, llk_q, llk_c, reads


@functools.lru_cache(maxsize=None)
def host(name, errors, flat=False):
    from mchap_amd import application

    KP, KQ, H = SHAPES[name]
    fr, llk_p, llk_q, llk_c, reads = inputs(name)
    out = []
    for r in range(3):
        F = None if flat else FS[r]
        progeny = [llk_c[r][c] if reads[r, c] else None for c in range(N_PROGENY)]
        out.append(application.family_unit(llk_p[r], KP, F, llk_q[r], KQ, F, H, fr[r], errors, progeny))
    return out


def device(name, errors, order=(0, 1, 2), flat=False, llk_p=None, **kw):
    """One call with the records in `order` -> the dict of host arrays, in the order given."""
    import torch

    from mchap_amd.device import ExactFamily

    KP, KQ, H = SHAPES[name]
    fr, base_p, llk_q, llk_c, reads = inputs(name)
    llk_p = base_p if llk_p is None else llk_p
    dev = ExactFamily()
    order = list(order)
    up = lambda tables: torch.from_numpy(np.ascontiguousarray(np.concatenate(tables))).to(dev.device)  # noqa: E731
    Fs = None if flat else [FS[r] for r in order]
    got = dev.call(up([llk_p[r] for r in order]), up([llk_q[r] for r in order]), up([llk_c[r][c] for r in order for c in range(N_PROGENY)]),
                   H, KP, KQ, fr[order], errors, Fs, Fs, reads[order], full=True, **kw)
    torch.cuda.synchronize()
    assert dev.launches == 1
    return {k: v.cpu().numpy() for k, v in got.items()}


def check(name, errors, flat=False, **kw):
    want = host(name, errors, flat)
    got = device(name, errors, flat=flat, **kw)
    worst = 0.0
    for r in range(3):
        w = want[r]
        pairs = [(got["post_p"][r], w["post_p"], "post_p"), (got["post_q"][r], w["post_q"], "post_q")]
        pairs += [(got["q"][r, c], w["q"][c], "q%d" % c) for c in range(N_PROGENY)]
        for g, h, key in pairs:
            ok, err = within(g, h)
            assert ok, (name, errors, r, key, err)
            worst = max(worst, err)
            assert abs(g.sum() - 1.0) <= 1e-9
        assert np.isfinite(w["log_z"]) and abs(got["log_z"][r] - w["log_z"]) <= LOG_TOL * max(1.0, abs(w["log_z"]))
        assert np.all(np.abs(got["pred"][r] - w["pred"]) <= LOG_TOL * np.maximum(1.0, np.abs(w["pred"])))
        assert got["pred"][r, NO_READS] == 0.0
        # modes: the first maximum of the device's own array, and the host's mode (or one within the bound of it)
        modes = [(got["mode_p"][r], got["prob_p"][r], got["post_p"][r], w["post_p"], w["mode_p"]),
                 (got["mode_q"][r], got["prob_q"][r], got["post_q"][r], w["post_q"], w["mode_q"])]
        modes += [(got["mode_c"][r, c], got["prob_c"][r, c], got["q"][r, c], w["q"][c], w["modes"][c]) for c in range(N_PROGENY)]
        for mode, prob, own, hq, hmode in modes:
            assert mode == int(np.argmax(own)) and prob == own[mode]
            assert mode == hmode or hq[hmode] - hq[mode] <= ref.REL * hq[hmode] + ref.FLOOR
    return worst


@pytest.mark.parametrize("errors", ERRORS)
@pytest.mark.parametrize("name", SHAPES)
def test_the_entry_point_against_the_host_definition(name, errors):
    worst = check(name, errors)
    if errors == (0.0, 0.0):
        assert any(np.any(w["q"][0] == 0.0) for w in host(name, errors))      # one-hot parents: exact zeros
    print("%s e=%r: worst |deviation| %.3g (REL %g, FLOOR %.3g)" % (name, errors, worst, ref.REL, ref.FLOOR))


@pytest.mark.parametrize("name", ["4x2-H4-unequal-parents", "4x4-H6-126x126-pairs"])
def test_the_flat_genotype_prior(name):
    check(name, (0.01, 0.05), flat=True)


@pytest.mark.parametrize("name", ["4x2-H4-unequal-parents", "6x6-H4-84x84-pairs", "10x8-H3-first-of-KM16"])
def test_the_forced_fallback_gives_equal_bits(name):
    check(name, (0.01, 0.05), force_fallback=True)
    base, other = device(name, (0.01, 0.05)), device(name, (0.01, 0.05), force_fallback=True)
    for key in base:
        assert base[key].tobytes() == other[key].tobytes(), key


@pytest.mark.parametrize("name", ["4x4-H6-126x126-pairs", "8x8-H3-last-of-KM8"])
def test_permuted_records_give_equal_bits(name):
    base, again = device(name, (0.01, 0.05)), device(name, (0.01, 0.05))
    got = device(name, (0.01, 0.05), order=(2, 0, 1))
    for key in base:
        assert base[key].tobytes() == again[key].tobytes(), key
        assert base[key][[2, 0, 1]].tobytes() == got[key].tobytes(), key


def test_a_parent_without_a_finite_genotype_and_its_neighbours():
    name = "4x4-H6-126x126-pairs"
    _, llk_p, _, _, _ = inputs(name)
    base = device(name, (0.01, 0.05))
    got = device(name, (0.01, 0.05), llk_p=[llk_p[0], np.full(len(llk_p[1]), -np.inf), llk_p[2]])
    assert np.all(np.isnan(got["post_p"][1])) and np.all(np.isnan(got["post_q"][1])) and np.all(np.isnan(got["q"][1]))
    assert not np.isfinite(got["log_z"][1]) and got["mode_p"][1] == -1 and got["mode_q"][1] == -1 and np.all(got["mode_c"][1] == -1)
    assert np.isnan(got["prob_p"][1]) and np.isnan(got["prob_q"][1]) and np.all(np.isnan(got["prob_c"][1])) and np.all(np.isnan(got["pred"][1]))
    for key in base:
        assert base[key][[0, 2]].tobytes() == got[key][[0, 2]].tobytes(), key


def test_no_progeny_gives_the_parents_own_posteriors():
    import torch

    from mchap_amd import application
    from mchap_amd.device import ExactFamily

    name = "4x2-H4-unequal-parents"
    KP, KQ, H = SHAPES[name]
    fr, llk_p, llk_q, _, _ = inputs(name)
    dev = ExactFamily()
    up = lambda tables: torch.from_numpy(np.ascontiguousarray(np.concatenate(tables))).to(dev.device)  # noqa: E731
    got = dev.call(up(llk_p), up(llk_q), None, H, KP, KQ, fr, (0.01, 0.05), FS, None)
    for r in range(3):
        assert within(got["post_p"][r].cpu().numpy(), application._unit_posterior(llk_p[r], H, KP, FS[r], fr[r])[0])[0]
        assert within(got["post_q"][r].cpu().numpy(), application._unit_posterior(llk_q[r], H, KQ, None, fr[r])[0])[0]
    assert tuple(got["pred"].shape) == (3, 0)


def test_a_workspace_one_byte_short_and_the_refused_shapes():
    import torch

    from mchap_amd import _lib
    from mchap_amd.device import ExactFamily, _ptr

    L = _lib.lib()
    assert ExactFamily.workspace_bytes(1, 5, 3, 4) == -1 and ExactFamily.workspace_bytes(1, 5, 16, 4) == -1
    assert ExactFamily.workspace_bytes(1, 3000, 14, 14) == -1
    need = ExactFamily.workspace_bytes(2, 4, 4, 4)
    assert 0 < need < ExactFamily.workspace_bytes(2, 4, 4, 4, force_fallback=True)
    dev = ExactFamily()
    G, H = comb(4 + 3, 4), 4
    d = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev.device)     # noqa: E731
    i = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev.device)       # noqa: E731
    llk, fr, err = d(2 * G), torch.full((2, H), 0.25, dtype=torch.float64, device=dev.device), d(2)
    outs = [d(2, G), i(2), d(2), d(2, G), i(2), d(2)]
    ws = torch.empty(need, dtype=torch.uint8, device=dev.device)

    def call(offered):
        return L.mchap_exact_family_device(2, 0, _ptr(llk), _ptr(llk), None, None, H, 4, 4, None, None, _ptr(fr), H, _ptr(err), _ptr(err),
                                           *[_ptr(t) for t in outs], None, None, None, None, _ptr(d(2)), _ptr(ws), C.c_int64(offered), 0, None)

    assert call(need - 1) == _lib.ERR_LIMIT
    assert call(need) == 0
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError):
        dev.call(llk, llk, None, H, 4, 4, fr, workspace_limit=need - 1)
    for bad in (1.5, -1e-9, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            dev.call(llk, llk, None, H, 4, 4, fr, (bad, 0.0))
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        dev.call(llk, llk, None, H, 4, 4, fr, inbreeding_p=1.0)
    assert dev.launches == 0


def test_the_calling_function():
    from mchap_amd import application, calling

    name = "4x2-H4-unequal-parents"
    KP, KQ, H = SHAPES[name]
    fr, llk_p, llk_q, llk_c, _ = inputs(name)
    post_p, post_q, q, log_z, pred = calling.family_genotype_posteriors(llk_p[0], KP, llk_q[0], KQ, llk_c[0], H, gamete_error=(0.01, 0.05),
                                                                         frequencies=fr[0])
    want = application.family_unit(llk_p[0], KP, None, llk_q[0], KQ, None, H, fr[0], (0.01, 0.05), llk_c[0])
    assert within(post_p, want["post_p"])[0] and within(post_q, want["post_q"])[0] and len(q) == N_PROGENY
    assert all(within(a, b)[0] for a, b in zip(q, want["q"]))
    assert abs(log_z - want["log_z"]) <= LOG_TOL * max(1.0, abs(want["log_z"])) and np.allclose(pred, want["pred"], rtol=0, atol=1e-8)
