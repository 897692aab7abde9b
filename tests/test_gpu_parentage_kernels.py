"""The kernels of the parentage evidence -- parentage_cw_kernel, parentage_max_kernel, parentage_w_kernel<2|4|7>, parentage_z_kernel,
parentage_mult_kernel -- driven through device.ExactParentage on drawn tables, against the float64 host definition
(application.parentage_unit; tests/test_parentage_reference.py holds it to long double, to the cross evidence through the cross
prior and to the reference's fixture on the CPU).  The bound on a log evidence: |got - want| <= 1e-9 |want| + 8 x ENVELOPE
(tests/parentage_reference.py); -inf, NaN and the exact 0 of a progeny without reads must match exactly.  Every launch holds 3
records x 3 progeny; the rows cycle through random candidates (record 0 under a zero frequency), one-hot candidates at a gamete
error of 0, and a candidate without reads."""
import ctypes as C
import functools
import zlib
from math import comb

import numpy as np
import pytest

from tests import parentage_reference as ref

pytestmark = pytest.mark.gpu

COLS = 16   # the kernel's column chunk (exact_parentage_kernel.hpp PARENTAGE_COLS): 19 rows a side cross it
# every shape with three rows a side; one row and nineteen on the shapes where another path is taken: progeny side by side in a
# workgroup (NA <= 128), two tiles of gametes, unequal gamete sizes, the unrolled loops of 2, 4 and 7
CASES = [(name, 3) for name in ref.SHAPES] + [(name, n) for n in (1, 19) for name in ("2x2-H3", "1x1-H91", "2x2-H23", "2x1-H4", "5x4-H3")] + \
    [("3x3-H12", 19)]


@functools.lru_cache(maxsize=None)
def case(name, n):
    return ref.draw_case(name, n=n, n_progeny=3, records=3)


@functools.lru_cache(maxsize=None)
def host(name, n):
    """float64 [3, 3, n, n]: the host definition of every (record, progeny)."""
    from mchap_amd import application

    t_a, t_b, H, gam_a, gam_b, llk, _ = case(name, n)
    return np.stack([np.stack([application.parentage_unit(gam_a[r], gam_b[r], llk[r, c], H, t_a, t_b) for c in range(3)]) for r in range(3)])


def device(t_a, t_b, H, gam_a, gam_b, llk, reads=None):
    """One launch -> log_z [R, C, n_a, n_b] on the host."""
    import torch

    from mchap_amd.device import ExactParentage

    dev = ExactParentage()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev.device)  # noqa: E731
    got = dev.log_evidence(up(gam_a), up(gam_b), up(llk).reshape(-1), H, t_a, t_b, reads)
    torch.cuda.synchronize()
    assert dev.launches == 1
    return got.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name, n", CASES, ids=["%s-n%d" % c for c in CASES])
def test_against_the_host_definition(name, n):
    t_a, t_b, H, gam_a, gam_b, llk, _ = case(name, n)
    got = device(t_a, t_b, H, gam_a, gam_b, llk)
    want = host(name, n)
    ok, err = ref.within(got, want)
    print("%s n=%d: largest |device - host| of a log evidence %.3g, entries at -inf %d" % (name, n, err, int(np.sum(want == -np.inf))))
    assert ok, (name, n, err)
    assert np.all(np.isfinite(want) | (want == -np.inf))


@pytest.mark.parametrize("name", ["2x2-H3", "2x1-H4"])
def test_every_entry_against_the_cross_prior_and_posterior_launches(name):
    """The path to the same numbers that exists without this kernel: ExactCross.cross_prior + posteriors, one pair at a time."""
    import torch

    from mchap_amd.device import ExactCross, ExactParentage

    t_a, t_b, H = ref.SHAPES[name]
    KP, KQ, n = 2 * t_a, 2 * t_b, 3
    rng = np.random.default_rng(zlib.crc32(("gpu-parentage-cross-%s" % name).encode()))
    fr = rng.dirichlet(np.full(H, 2.0), size=3)
    par, cross = ExactParentage(), ExactCross()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(par.device)  # noqa: E731
    rows = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    gam = {K: par.gametes(up(-rng.exponential(4.0, size=(9, comb(H + K - 1, K)))).reshape(-1), H, K, None, rows, fr, 0.01).view(3, n, -1)
           for K in {KP, KQ}}
    llk = up(-rng.exponential(4.0, size=(3, 3, comb(H + t_a + t_b - 1, t_a + t_b))))
    got = par.log_evidence(gam[KP].contiguous(), gam[KQ].contiguous(), llk.reshape(-1), H, t_a, t_b).cpu().numpy()
    for i in range(n):
        for j in range(n):
            log_x = cross.cross_prior(gam[KP][:, i].contiguous(), gam[KQ][:, j].contiguous(), H, KP, KQ)
            log_z = cross.posteriors(llk.reshape(-1), H, t_a + t_b, log_x, rows)[0].cpu().numpy().reshape(3, 3)
            ok, err = ref.within(got[:, :, i, j], log_z)
            assert ok, (name, i, j, err)


def test_the_same_table_on_both_sides_is_symmetric_within_the_bound():
    t_a, t_b, H, gam_a, _, llk, _ = case("2x2-H23", 19)
    got = device(t_a, t_b, H, gam_a, gam_a, llk)
    ok, err = ref.within(got, np.swapaxes(got, 2, 3))
    assert ok, err


def test_equal_bits_whatever_the_place_and_the_company():
    name, n = "2x2-H23", 19
    t_a, t_b, H, gam_a, gam_b, llk, _ = case(name, n)
    first = device(t_a, t_b, H, gam_a, gam_b, llk)
    assert np.array_equal(bits(first), bits(device(t_a, t_b, H, gam_a, gam_b, llk)))                       # twice over
    assert np.array_equal(bits(first[::-1]), bits(device(t_a, t_b, H, gam_a[::-1], gam_b[::-1], llk[::-1])))   # reversed records
    rng = np.random.default_rng(5)
    pa, pb, pc = rng.permutation(n), rng.permutation(n), np.array([2, 0, 1])
    assert np.array_equal(bits(first[:, :, pa][:, :, :, pb]), bits(device(t_a, t_b, H, gam_a[:, pa], gam_b[:, pb], llk)))   # permuted candidates
    assert np.array_equal(bits(first[:, pc]), bits(device(t_a, t_b, H, gam_a, gam_b, llk[:, pc])))         # permuted progeny
    # a call that holds only one of the candidates on either side, and one progeny of one record
    for i, j in ((0, 0), (4, 17), (18, 16)):
        alone = device(t_a, t_b, H, gam_a[1:2, i:i + 1], gam_b[1:2, j:j + 1], llk[1:2, 2:3])
        assert bits(alone)[0, 0, 0, 0] == bits(first)[1, 2, i, j]
    # ... and with the progeny side by side in a workgroup
    t_a, t_b, H, gam_a, gam_b, llk, _ = case("2x1-H4", 19)
    first = device(t_a, t_b, H, gam_a, gam_b, llk)
    alone = device(t_a, t_b, H, gam_a[2:3, 3:4], gam_b[2:3, 17:18], llk[2:3, 1:2])
    assert bits(alone)[0, 0, 0, 0] == bits(first)[2, 1, 3, 17]
    assert np.array_equal(bits(first[:, pc]), bits(device(t_a, t_b, H, gam_a, gam_b, llk[:, pc])))


def test_a_nan_candidate_leaves_its_neighbours_bits_untouched():
    t_a, t_b, H, gam_a, gam_b, llk, _ = case("2x2-H23", 19)
    first = device(t_a, t_b, H, gam_a, gam_b, llk)
    bad_a, bad_b = gam_a.copy(), gam_b.copy()
    bad_a[1, 4], bad_b[2, 17] = np.nan, np.nan
    got = device(t_a, t_b, H, bad_a, bad_b, llk)
    nan = np.zeros(got.shape, dtype=bool)
    nan[1, :, 4, :] = True
    nan[2, :, :, 17] = True
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(first[~nan]))
    # a progeny with a NaN likelihood, and one without a finite likelihood: NaN throughout, and nowhere else
    bad = llk.copy()
    bad[0, 1, 7] = np.nan
    bad[2, 0, :] = -np.inf
    got = device(t_a, t_b, H, gam_a, gam_b, bad)
    nan = np.zeros(got.shape, dtype=bool)
    nan[0, 1], nan[2, 0] = True, True
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(first[~nan]))


def test_one_hot_parents_that_cannot_make_the_progeny_give_minus_infinity():
    from mchap_amd import application

    H, G = 3, comb(3 + 3, 4)
    p0, p2 = np.zeros(G), np.zeros(G)
    p0[0], p2[G - 1] = 1.0, 1.0                      # 0/0/0/0 and 2/2/2/2 at a gamete error of 0
    f = np.full(H, 1.0 / H)
    rows = np.stack([application.gamete_table(p, H, 4, f, 0.0) for p in (p0, p2)])[None]
    llk = np.full((1, 2, G), -np.inf)
    llk[0, 0, application._multiset_ranks(np.array([[1, 1, 1, 1]]))[0]] = -1.0      # a progeny neither pair can make
    llk[0, 1, application._multiset_ranks(np.array([[0, 0, 2, 2]]))[0]] = -1.0      # one that only the pair (0, 1) makes
    got = device(2, 2, H, rows, rows, llk)
    assert np.all(got[0, 0] == -np.inf)
    assert got[0, 1, 0, 0] == -np.inf and got[0, 1, 1, 1] == -np.inf and got[0, 1, 0, 1] == got[0, 1, 1, 0] == -1.0


def test_a_progeny_without_reads_is_exactly_zero_and_is_not_read():
    t_a, t_b, H, gam_a, gam_b, llk, _ = case("2x2-H3", 3)
    first = device(t_a, t_b, H, gam_a, gam_b, llk)
    reads = np.array([[1, 0, 1], [1, 1, 1], [0, 1, 0]], dtype=np.int32)
    blank = llk.copy()
    blank[reads == 0] = np.nan                       # (what a read of them would show)
    bad_a = gam_a.copy()
    bad_a[2, 1] = np.nan                             # (a NaN candidate beside them: still exactly 0)
    got = device(t_a, t_b, H, bad_a, gam_b, blank, reads)
    assert np.array_equal(bits(got[reads == 0]), bits(np.zeros_like(got[reads == 0])))
    keep = (reads == 1)[:, :, None, None] & np.ones(got.shape, dtype=bool)
    keep[2, :, 1, :] = False
    assert np.array_equal(bits(got[keep]), bits(first[keep])) and np.all(np.isnan(got[2, 1, 1, :]))


def test_the_population_row_and_the_table():
    import torch

    from mchap_amd import application
    from mchap_amd.device import ExactParentage

    dev = ExactParentage()
    for name in ("1x1-H91", "2x2-H23", "7x7-H2", "3x3-H12"):
        t, _, H = ref.SHAPES[name]
        fr = case(name, 3)[6]
        want = np.stack([application.population_gametes(H, t, f) for f in fr])
        assert np.array_equal(bits(dev.population(fr, H, t).cpu().numpy()), bits(want))           # products alone: the same bits
        rows = torch.from_numpy(case(name, 3)[3]).to(dev.device)
        table = dev.table(rows, fr, H, t).cpu().numpy()
        assert table.shape == (3, 4, want.shape[1])
        assert np.array_equal(bits(table[:, :3]), bits(case(name, 3)[3])) and np.array_equal(bits(table[:, 3]), bits(want))
        assert np.array_equal(bits(dev.table(None, fr, H, t).cpu().numpy()[:, 0]), bits(want))
        assert abs(want[1].sum() - 1.0) <= 1e-12


def test_a_workspace_one_byte_short_and_the_refused_shapes():
    import torch

    from mchap_amd import _lib
    from mchap_amd.device import ExactParentage, _ptr

    L = _lib.lib()
    wb = ExactParentage.workspace_bytes
    assert wb(1, 1, 1, 1, 4, 0, 2) == -1 and wb(1, 1, 1, 1, 4, 2, 8) == -1          # a gamete size outside 1..7
    assert wb(1, 1, 1, 1, 100000, 7, 7) == -1                                       # 2^62 genotypes
    assert wb(1, 1, 1, 1, 20000, 1, 1) == -1                                        # the rank table beyond the LDS
    assert wb(1, 1, 1, 1, 4, 7, 7) > 0 and wb(0, 3, 1, 1, 4, 2, 2) == 0
    t_a, t_b, H, gam_a, gam_b, llk, _ = case("2x2-H3", 3)
    need = wb(3, 3, 3, 3, H, t_a, t_b)
    assert need >= 3 * 3 * 3 * comb(H + 1, 2) * 8
    dev = ExactParentage()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev.device)  # noqa: E731
    A, B, c = up(gam_a), up(gam_b), up(llk)
    out = torch.empty((3, 3, 3, 3), dtype=torch.float64, device=dev.device)
    ws = torch.empty(need, dtype=torch.uint8, device=dev.device)

    def call(offered, ta=t_a, tb=t_b):
        return L.mchap_exact_parentage_device(3, 3, 3, 3, _ptr(A), _ptr(B), _ptr(c), None, H, ta, tb, _ptr(out), _ptr(ws), C.c_int64(offered), None)

    assert call(need - 1) == _lib.ERR_LIMIT
    assert call(need, 8, 2) == _lib.ERR_LIMIT and call(need, 2, 0) == _lib.ERR_LIMIT
    assert call(need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(device(t_a, t_b, H, gam_a, gam_b, llk)))
    with pytest.raises(NotImplementedError):
        dev.log_evidence(A, B, c.reshape(-1), H, t_a, t_b, workspace_limit=need - 1)
    with pytest.raises(NotImplementedError):
        dev.population(case("2x2-H3", 3)[6], H, 8)
    for bad in (1.5, -1e-9, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            dev.gametes(up(np.zeros(comb(H + 3, 4))), H, 4, None, [0], case("2x2-H3", 3)[6], bad)


def test_the_calling_layer_takes_numpy_in_and_gives_numpy_out():
    from mchap_amd import calling

    t_a, t_b, H, gam_a, gam_b, llk, _ = case("2x1-H4", 3)
    got = calling.parentage_log_evidence(gam_a[0], gam_b[0], llk[0], H, t_a, t_b)
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(device(t_a, t_b, H, gam_a[:1], gam_b[:1], llk[:1])[0]))
    one = calling.parentage_log_evidence(gam_a[0, 1], gam_b[0, 2], llk[0, 1], H, t_a, t_b)
    assert one.shape == (1, 1) and bits(one)[0, 0] == bits(got)[1, 1, 2]
