"""The kernels of the selfing prior and its evidence -- exact_selfing_post_kernel, exact_selfing_prior_kernel<4|8|16>,
selfing_max_kernel, selfing_evidence_kernel, selfing_combine_kernel -- driven through device.ExactSelfing on drawn units, against the
float64 host definition (application.selfing_prior_unit, selfing_evidence; tests/test_selfing_reference.py holds it to long double
and to the reference's fixture on the CPU).  The bound: |got - want| <= 1e-9 |want| + 8 x ENVELOPE (tests/selfing_reference.py);
NaN where NaN, and the exact zeros, -inf and the exact 0 of a progeny without reads must match exactly.  A prior launch holds
every parent kind (random, one-hot, no reads, no finite genotype) at every gamete error (0, 0.01, 1), its units on different
frequency rows: one launch under the flat prior and one with F = 0 (on the row with a zero frequency) beside F = 0.3."""
import ctypes as C
import functools
import zlib
from math import comb

import numpy as np
import pytest

from tests import selfing_reference as ref
from tests.cross_reference import draw_frequencies, parent_llk, within

pytestmark = pytest.mark.gpu

# (K, H): G = 15, 15, 330 (more than one workgroup of 256 lanes, a ragged tail), 84, 45, 66 (exact_selfing_prior_kernel<16>)
SHAPES = [(2, 5), (4, 3), (4, 8), (6, 4), (8, 3), (10, 3)]
KINDS = ("random", "one-hot", "no-reads", "none-finite")
ERRORS = (0.0, 0.01, 1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def possible(H, K, f):
    from mchap_amd import application

    g = application._genotype_table(H, K)
    return np.nonzero(np.all(np.asarray(f)[g] > 0, axis=1))[0]


@functools.lru_cache(maxsize=None)
def units(K, H, prior):
    """(llks [U, G], F [U] or None, rows [U], freqs [3, H], errors [U]): every kind x every error."""
    rng = np.random.default_rng(zlib.crc32(("gpu-selfing-%d-%d-%s" % (K, H, prior)).encode()))
    G = comb(H + K - 1, K)
    fr = draw_frequencies(rng, H)
    llks, F, rows, errors = [], [], [], []
    for i, (kind, e) in enumerate((kind, e) for kind in KINDS for e in ERRORS):
        row = i % 3
        if prior == "flat":
            F.append(None)
        else:
            F.append(0.0 if row == 0 else 0.3)   # (row 0 holds a zero frequency)
        if kind == "none-finite":
            llk = np.full(G, -np.inf)
        elif kind == "one-hot" and prior != "flat" and row == 0:
            ok = possible(H, K, fr[0])
            llk = np.full(G, -np.inf)
            llk[ok[rng.integers(len(ok))]] = -3.0
        else:
            llk = parent_llk(rng, kind, G)
        llks.append(llk)
        rows.append(row)
        errors.append(e)
    return np.stack(llks), (None if prior == "flat" else np.array(F)), np.array(rows, dtype=np.int32), fr, np.array(errors)


@functools.lru_cache(maxsize=None)
def host(K, H, prior):
    """(S [U, G], log_norm [U]) of the host definition."""
    from mchap_amd import application

    llks, F, rows, fr, errors = units(K, H, prior)
    out = [application.selfing_prior_unit(llks[u], K, None if F is None else float(F[u]), H, fr[rows[u]], float(errors[u]))
           for u in range(len(llks))]
    return np.stack([o["S"] for o in out]), np.array([o["log_norm"] for o in out])


def device_prior(K, H, llks, F, rows, fr, errors):
    """One launch -> (log_self, self_prior, log_norm) on the host."""
    import torch

    from mchap_amd.device import ExactSelfing

    dev = ExactSelfing()
    d = torch.from_numpy(np.ascontiguousarray(llks, dtype=np.float64)).to(dev.device).reshape(-1)
    got = dev.selfing_prior(d, H, K, F, rows, fr, errors)
    torch.cuda.synchronize()
    assert dev.launches == 1
    return tuple(t.cpu().numpy() for t in got)


def gamete_norm(K, H, llks, F, rows, fr):
    """log_norm [U] of ExactCross.gametes on the same units."""
    import torch

    from mchap_amd.device import ExactCross

    dev = ExactCross()
    dev.gametes(torch.from_numpy(np.ascontiguousarray(llks, dtype=np.float64)).to(dev.device).reshape(-1), H, K, F, rows, fr, 0.0)
    return dev.log_norm.cpu().numpy()


def hold_prior(got, want_S, label):
    log_self, lin, _ = got
    ok, err = within(lin, want_S, ref.FLOOR)
    assert ok, (label, err)
    with np.errstate(divide="ignore"):
        want_log = np.log(want_S)
    assert np.array_equal(np.isnan(log_self), np.isnan(want_log)) and np.array_equal(log_self == -np.inf, want_log == -np.inf), label
    live = np.isfinite(want_log)
    assert np.all(np.abs(log_self[live] - want_log[live]) <= ref.REL * np.abs(want_log[live]) + ref.FLOOR), label
    return err


@pytest.mark.parametrize("prior", ["flat", "F"])
@pytest.mark.parametrize("K, H", SHAPES, ids=["K%d-H%d" % s for s in SHAPES])
def test_the_prior_against_the_host_definition(K, H, prior):
    llks, F, rows, fr, errors = units(K, H, prior)
    want_S, want_norm = host(K, H, prior)
    got = device_prior(K, H, llks, F, rows, fr, errors)
    err = hold_prior(got, want_S, (K, H, prior))
    dead = np.isnan(want_S[:, 0])
    print("K%d-H%d %s: largest |device - host| of S %.3g; exact zeros %d; NaN units %d" % (K, H, prior, err, int(np.sum(want_S == 0.0)), int(dead.sum())))
    assert dead.sum() == len(ERRORS)                                   # the units without a finite genotype, and no other
    assert np.all(np.abs(np.nansum(got[1], axis=1)[~dead] - 1.0) <= 1e-12)
    # log_norm is not formed by these kernels: it is the gamete launch's normaliser (the model-evidence launch at the unit's own F),
    # copied.  Bit for bit that launch's, and within the bound tests/test_gpu_cross_kernels.py holds that launch to (LOG_TOL there:
    # a relative deviation of the evidence itself and the rounding of the logarithm -- the envelope of S says nothing about it)
    assert np.array_equal(bits(got[2]), bits(gamete_norm(K, H, llks, F, rows, fr)))
    live = np.isfinite(want_norm)
    assert np.array_equal(np.isfinite(got[2]), live)
    assert np.all(np.abs(got[2][live] - want_norm[live]) <= 2e-9 * np.maximum(1.0, np.abs(want_norm[live])))
    at_one = (errors == 1.0) & ~dead                                   # e = 1: the population's multinomial, bit for bit
    from mchap_amd import application
    for u in np.nonzero(at_one)[0]:
        assert np.array_equal(bits(got[1][u]), bits(application.population_gametes(H, K, fr[rows[u]])))


def test_one_unit_of_sixteen_haplotypes():
    """Tetraploid over 16 haplotypes, G = 3876: sixteen workgroups of one unit, the trip counts of a realistic record."""
    from mchap_amd import application

    K, H = 4, 16
    rng = np.random.default_rng(416)
    G = comb(H + K - 1, K)
    fr = draw_frequencies(rng, H)
    llk = -rng.exponential(4.0, size=(1, G))
    want = application.selfing_prior_unit(llk[0], K, 0.3, H, fr[1], 0.01)
    got = device_prior(K, H, llk, np.array([0.3]), np.array([1], dtype=np.int32), fr, np.array([0.01]))
    err = hold_prior(got, want["S"][None], "K4-H16")
    print("K4-H16: largest |device - host| of S %.3g" % err)
    assert abs(got[1].sum() - 1.0) <= 1e-12


def test_the_prior_has_equal_bits_whatever_the_place_and_the_batch():
    K, H = 4, 8
    llks, F, rows, fr, errors = units(K, H, "F")
    first = device_prior(K, H, llks, F, rows, fr, errors)
    again = device_prior(K, H, llks, F, rows, fr, errors)
    perm = np.random.default_rng(3).permutation(len(llks))
    moved = device_prior(K, H, llks[perm], F[perm], rows[perm], fr, errors[perm])
    for a, b, c in zip(first, again, moved):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a[perm]), bits(c))
    for u in (0, 4, 7):                                                # a batch of one
        alone = device_prior(K, H, llks[u:u + 1], F[u:u + 1], rows[u:u + 1], fr, errors[u:u + 1])
        for a, b in zip(first, alone):
            assert np.array_equal(bits(a[u:u + 1]), bits(b))


# ---- the evidence launch: drawn rows S; (K, H, n): one tile; G = 4845, two tiles with a ragged tail ----
EVIDENCE = [(4, 3, 3), (6, 4, 5), (4, 17, 3)]


@functools.lru_cache(maxsize=None)
def evidence_case(K, H, n, R=3, Cn=3):
    rng = np.random.default_rng(zlib.crc32(("gpu-selfing-evidence-%d-%d-%d" % (K, H, n)).encode()))
    G = comb(H + K - 1, K)
    S = rng.dirichlet(np.full(G, 0.5), size=(R, n))
    S[0, 0, rng.random(G) < 0.5] = 0.0
    llk = -rng.exponential(4.0, size=(R, Cn, G)) * 6.0
    return S, llk


def device_evidence(K, H, S, llk, reads=None):
    import torch

    from mchap_amd.device import ExactSelfing

    dev = ExactSelfing()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev.device)  # noqa: E731
    got = dev.log_evidence(up(S), up(llk).reshape(-1), H, K, reads)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def host_evidence(S, llk):
    from mchap_amd import application

    return np.stack([np.stack([application.selfing_evidence(S[r], llk[r, c]) for c in range(llk.shape[1])]) for r in range(len(S))])


@pytest.mark.parametrize("K, H, n", EVIDENCE, ids=["K%d-H%d-n%d" % s for s in EVIDENCE])
def test_the_evidence_against_the_host_definition(K, H, n):
    S, llk = evidence_case(K, H, n)
    got, want = device_evidence(K, H, S, llk), host_evidence(S, llk)
    ok, err = within(got, want, ref.FLOOR)
    print("K%d-H%d n=%d: largest |device - host| of a log evidence %.3g" % (K, H, n, err))
    assert ok, err
    direct = np.log(np.einsum("rng,rcg->rcn", S, np.exp(llk)))
    assert np.all(np.abs(want - direct) <= 1e-9 * np.abs(direct))


def test_the_evidence_of_the_prior_launch_end_to_end():
    """Both launches in a row against selfing_prior_unit's log_z."""
    from mchap_amd import application

    K, H = 6, 4
    llks, F, rows, fr, errors = units(K, H, "F")
    keep = [u for u in range(len(llks)) if rows[u] == 1][:3]          # three candidates of one record (one frequency row)
    S = device_prior(K, H, llks[keep], F[keep], rows[keep], fr, errors[keep])[1]
    llk_c = -np.random.default_rng(8).exponential(4.0, size=(1, 2, S.shape[1]))
    got = device_evidence(K, H, S[None], llk_c)
    for c in range(2):
        for i, u in enumerate(keep):
            want = application.selfing_prior_unit(llks[u], K, float(F[u]), H, fr[1], float(errors[u]), llk_c[0, c])["log_z"]
            if np.isnan(want):
                assert np.isnan(got[0, c, i])
            else:
                assert abs(got[0, c, i] - want) <= ref.REL * abs(want) + ref.FLOOR


def test_the_evidence_has_equal_bits_whatever_the_place_and_the_company():
    K, H, n = 4, 17, 3
    S, llk = evidence_case(K, H, n)
    first = device_evidence(K, H, S, llk)
    assert np.array_equal(bits(first), bits(device_evidence(K, H, S, llk)))
    assert np.array_equal(bits(first[::-1]), bits(device_evidence(K, H, S[::-1], llk[::-1])))
    pn, pc = np.array([2, 0, 1]), np.array([1, 2, 0])
    assert np.array_equal(bits(first[:, :, pn]), bits(device_evidence(K, H, S[:, pn], llk)))
    assert np.array_equal(bits(first[:, pc]), bits(device_evidence(K, H, S, llk[:, pc])))
    alone = device_evidence(K, H, S[1:2, 2:3], llk[1:2, 0:1])
    assert bits(alone)[0, 0, 0] == bits(first)[1, 0, 2]


def test_no_reads_nan_and_minus_infinity_in_the_evidence():
    K, H, n = 4, 3, 3
    S, llk = evidence_case(K, H, n)
    first = device_evidence(K, H, S, llk)
    reads = np.array([[1, 0, 1], [1, 1, 1], [0, 1, 0]], dtype=np.int32)
    blank = llk.copy()
    blank[reads == 0] = np.nan                                         # (what a read of them would show)
    bad = S.copy()
    bad[2, 1] = np.nan                                                 # a NaN candidate row poisons its column alone
    got = device_evidence(K, H, bad, blank, reads)
    assert np.array_equal(bits(got[reads == 0]), bits(np.zeros_like(got[reads == 0])))
    keep = (reads == 1)[:, :, None] & np.ones(got.shape, dtype=bool)
    keep[2, :, 1] = False
    assert np.array_equal(bits(got[keep]), bits(first[keep])) and np.isnan(got[2, 1, 1])
    # a progeny with a NaN likelihood, and one without a finite likelihood: NaN throughout, and nowhere else
    worse = llk.copy()
    worse[0, 1, 7] = np.nan
    worse[2, 0, :] = -np.inf
    got = device_evidence(K, H, S, worse)
    nan = np.zeros(got.shape, dtype=bool)
    nan[0, 1], nan[2, 0] = True, True
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(first[~nan]))
    # a prior that excludes every genotype the reads allow: exactly -inf
    one = np.zeros((1, 1, S.shape[2]))
    one[0, 0, 0] = 1.0
    only = np.full((1, 1, S.shape[2]), -np.inf)
    only[0, 0, 3] = -1.0
    assert device_evidence(K, H, one, only)[0, 0, 0] == -np.inf


def test_refused_shapes_and_short_workspaces():
    import torch

    from mchap_amd import _lib
    from mchap_amd.device import ExactSelfing, _ptr

    L = _lib.lib()
    pw, ew = ExactSelfing.prior_workspace_bytes, ExactSelfing.evidence_workspace_bytes
    assert pw(1, 4, 18) == -1 and pw(1, 100000, 14) == -1              # the ploidy, 2^62 genotypes
    assert pw(1, 5000, 2) == -1                                        # the rank table beyond 64 KB of LDS
    assert pw(0, 4, 4) == 0 and pw(3, 4, 4) > 3 * 35 * 8
    assert ew(1, 1, 1, 4, 18) == -1 and ew(1, 1, 1, 100000, 14) == -1 and ew(0, 1, 1, 4, 4) == 0 and ew(2, 2, 2, 4, 4) > 0
    K, H = 4, 3
    llks, F, rows, fr, errors = units(K, H, "F")
    U, G = llks.shape
    dev = ExactSelfing()
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev.device)  # noqa: E731
    d_llk, d_F, d_row, d_fr, d_e = up(llks), up(F), up(rows, np.int32), up(fr), up(errors)
    out, lin = (torch.empty((U, G), dtype=torch.float64, device=dev.device) for _ in range(2))
    need = pw(U, H, K)
    ws = torch.empty(need, dtype=torch.uint8, device=dev.device)

    def call(offered, haps=H, ploidy=K):
        return L.mchap_exact_selfing_prior_device(U, _ptr(d_llk), haps, ploidy, _ptr(d_F), _ptr(d_row), _ptr(d_fr), H, _ptr(d_e), _ptr(out),
                                                  _ptr(lin), None, _ptr(ws), C.c_int64(offered), None)

    assert call(need - 1) == _lib.ERR_BAD_ARG                          # (as the gamete entry: nothing is allocated behind the caller)
    assert call(need, H, 18) == _lib.ERR_LIMIT and call(need, H, 3) == _lib.ERR_BAD_ARG
    assert call(need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(lin.cpu().numpy()), bits(device_prior(K, H, llks, F, rows, fr, errors)[1]))
    with pytest.raises(NotImplementedError):
        dev.selfing_prior(d_llk.reshape(-1), H, K, F, rows, fr, errors, workspace_limit=need - 1)
    for bad in (1.5, -1e-9, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            dev.selfing_prior(d_llk.reshape(-1), H, K, F, rows, fr, bad)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        dev.selfing_prior(d_llk.reshape(-1), H, K, 1.0, rows, fr, 0.01)
    S, llk = evidence_case(4, 3, 3)
    d_S, d_c = up(S), up(llk)
    z = torch.empty((3, 3, 3), dtype=torch.float64, device=dev.device)
    need = ew(3, 3, 3, 3, 4)
    ws = torch.empty(need, dtype=torch.uint8, device=dev.device)
    ev = lambda offered, ploidy=4: L.mchap_exact_selfing_evidence_device(3, 3, 3, _ptr(d_S), _ptr(d_c), None, 3, ploidy, _ptr(z), _ptr(ws),  # noqa: E731
                                                                        C.c_int64(offered), None)
    assert ev(need - 1) == _lib.ERR_LIMIT and ev(need, 18) == _lib.ERR_LIMIT and ev(need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(z.cpu().numpy()), bits(device_evidence(4, 3, S, llk)))
    with pytest.raises(NotImplementedError):
        dev.log_evidence(d_S, d_c.reshape(-1), 3, 4, workspace_limit=need - 1)


def test_the_calling_layer_takes_numpy_in_and_gives_numpy_out():
    from mchap_amd import application, calling

    K, H = 4, 3
    rng = np.random.default_rng(12)
    G = comb(H + K - 1, K)
    post = rng.dirichlet(np.ones(G), size=2)
    f = rng.dirichlet(np.full(H, 2.0))
    got = calling.selfing_genotype_prior(post, K, H, 0.01, f)
    assert isinstance(got, np.ndarray) and got.shape == (2, G)
    for i in range(2):
        ok, err = within(got[i], application.selfing_prior(post[i], K, H, f, 0.01), ref.FLOOR)
        assert ok, err
    bad = post.copy()
    bad[1, 3] = np.nan                                                 # a NaN posterior: NaN throughout, as the definition; its neighbour untouched
    again = calling.selfing_genotype_prior(bad, K, H, 0.01, f)
    assert np.all(np.isnan(again[1])) and np.array_equal(bits(again[0]), bits(got[0]))
    one = calling.selfing_genotype_prior(post[0], K, H)
    assert one.shape == (G,) and abs(one.sum() - 1.0) <= 1e-12
