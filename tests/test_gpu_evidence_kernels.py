"""The kernels of the model evidence -- exact_evidence_kernel<8|16>, exact_evidence_combine_kernel -- driven through
device.ExactModelEvidence with the synthetic likelihood tables of tests/estimate_cases.py, against the long-double reference
(tests/evidence_reference.py; tests/test_evidence_reference.py anchors it on the CPU): grids of one, three and seven F per unit, the
flat prior, the grid worked in chunks where the prior tables do not fit together, a table above 64 KB of LDS, and the properties that
need no reference -- normalised priors, shifts, a unit without a finite genotype, unit order, equal bits, the frequency rows'
layout -- the shipped caller's posteriors, and the entry's refusals."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

from tests import estimate_cases as cases
from tests import evidence_reference as ref

pytestmark = pytest.mark.gpu

GRID3 = ((0.0, 0.1, 1e-4), (0.5, 0.0, 0.99), (1e-3, 0.5, 0.0))
GRID7 = (0.0, 1e-4, 1e-3, 0.1, 0.0, 0.5, 0.99)
KINDS = ("own", "three", "seven", "flat")
# one table alone above 64 KB of LDS (the cases' `lds-above-64K` is named for the estimate's layout): K = 2, H = 1100
BIG = ("one-table-above-64K", 2, 1100)


def ev_lds_bytes(H, K, chunk):
    """exact_ev_lds (exact_kernel.hpp), restated."""
    return (256 * 17 + chunk * H * (K + 1) + (K + 1) + H + 8 + chunk) * 8


def ev_chunk(H, K, n_grid):
    """exact_ev_chunk, restated: grid points per chunk within 64 KB, at least one (up to 160 KB), 0 beyond."""
    if ev_lds_bytes(H, K, 1) > 160 * 1024:
        return 0
    c = 1
    while c < n_grid and ev_lds_bytes(H, K, c + 1) <= 64 * 1024:
        c += 1
    return c


def grid_of(kind, u, own):
    """The grid of unit u: its own F, a three-point or the seven-point grid rotated by u (F = 0 and F > 0 mixed, different per
    unit), or None (flat)."""
    if kind == "own":
        return (own,)
    if kind == "three":
        return GRID3[u % 3]
    if kind == "seven":
        return GRID7[u % 7:] + GRID7[:u % 7]
    return None


@functools.lru_cache(maxsize=None)
def case_units(name):
    """(H, K, freqs [records, H], units [(llk, record, own F)]) of a case."""
    if name == BIG[0]:
        _, K, H = BIG
        rng = np.random.default_rng(17)
        f = cases.frequency_row(rng, H, "top_two_zero")
        return H, K, np.stack([f]), [(cases.likelihood_table(rng, H, K, "holes", f), 0, 0.1),
                                     (cases.likelihood_table(rng, H, K, "uniform400", f), 0, 0.0)]
    K, H, _ = cases.CASES[name]
    records = cases.build_case(name)
    return H, K, np.stack([r["f"] for r in records]), [(llk, i, F) for i, r in enumerate(records) for llk, _, F in r["units"]]


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """[U][n_grid] long-double evidence of a case under a grid kind, computed once."""
    H, K, freqs, units = case_units(name)
    out = []
    for u, (llk, rec, own) in enumerate(units):
        g = grid_of(kind, u, own)
        out.append([ref.evidence(llk, H, K, F, freqs[rec]) for F in (g if g is not None else (None,))])
    return out


def run(H, K, tables, grids, rows=None, freqs=None):
    """device.ExactModelEvidence.add_group over `tables` -> float64 [U, n_grid] on the host."""
    import torch

    from mchap_amd.device import ExactModelEvidence

    ev = ExactModelEvidence()
    llks = torch.from_numpy(np.concatenate(tables)).to(ev.device)
    got = ev.add_group(llks, H, K, grids, rows, freqs)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def run_case(name, kind, order=None):
    H, K, freqs, units = case_units(name)
    order = list(range(len(units))) if order is None else list(order)
    grids = None if kind == "flat" else [grid_of(kind, u, units[u][2]) for u in order]
    return run(H, K, [units[u][0] for u in order], grids, [units[u][1] for u in order], freqs)


def check(name, kind, got, order=None):
    """Every value against the reference: (all within the bound, worst |got - want|)."""
    H, K, freqs, units = case_units(name)
    want = reference(name, kind)
    order = list(range(len(units))) if order is None else list(order)
    ok, worst = True, 0.0
    for i, u in enumerate(order):
        g = grid_of(kind, u, units[u][2])
        for n, F in enumerate(g if g is not None else (None,)):
            o, err = ref.within(got[i][n], want[u][n], F)
            ok, worst = ok and o, max(worst, err)
    return ok, worst


def test_the_grid_is_worked_in_chunks_where_the_tables_do_not_fit():
    from mchap_amd import _lib

    L = _lib.lib()
    shapes = [(K, H) for K, H, _ in cases.CASES.values()] + [(BIG[1], BIG[2]), (2, 4029), (2, 4030), (6, 500)]
    for K, H in shapes:
        for n in (1, 3, 7, 8):
            assert int(L.mchap_exact_evidence_chunk(H, K, n)) == ev_chunk(H, K, n), (K, H, n)
    assert 1 <= ev_chunk(500, 2, 7) < 7                       # lds-above-64K with seven points: several chunks
    assert ev_chunk(500, 2, 7) == 2 and ev_lds_bytes(500, 2, 2) <= 64 * 1024 < ev_lds_bytes(500, 2, 3)
    assert all(ev_chunk(H, K, 7) == 7 for K, H, _ in list(cases.CASES.values())[:-1])
    assert ev_chunk(BIG[2], BIG[1], 2) == 1 and ev_lds_bytes(BIG[2], BIG[1], 1) > 64 * 1024   # one table above 64 KB: the attribute
    assert ev_chunk(500, 6, 7) == 1 and ev_chunk(4029, 2, 7) == 1 and ev_chunk(4030, 2, 7) == 0


@pytest.mark.parametrize("name", list(cases.CASES) + [BIG[0]])
def test_the_kernels_against_long_double(name):
    H, K, freqs, units = case_units(name)
    for llk, rec, _ in units:   # on the CPU, before anything is launched: every unit keeps a finite genotype
        assert np.any(cases.prior_finite(H, K, freqs[rec]) & np.isfinite(llk))
    kinds = ("three", "flat") if name == BIG[0] else KINDS
    for kind in kinds:
        got = run_case(name, kind)
        assert got.shape == (len(units), {"own": 1, "three": 3, "seven": 7, "flat": 1}[kind])
        ok, worst = check(name, kind, got)
        print("%s, grid %s: worst |deviation| %.3g (REL %g, FLOOR 8 x envelope)" % (name, kind, worst, ref.REL))
        assert ok, (name, kind, worst, got.tolist(), reference(name, kind))


def test_a_chunk_of_more_grid_points_than_the_workgroup_has_threads():
    """A fine scan of F over a small shape: at H = 2, K = 2 the 64 KB rule lets 546 points share a chunk, more than twice the 256
    threads that build the chunk's constants; 600 points are a chunk of 546 and one of 54."""
    from mchap_amd import _lib

    H, K, n = 2, 2, 600
    assert int(_lib.lib().mchap_exact_evidence_chunk(H, K, n)) == ev_chunk(H, K, n) == 546
    rng = np.random.default_rng(23)
    freqs = np.stack([cases.frequency_row(rng, H, v) for v in cases.variants_for(H)])
    tables = [cases.likelihood_table(rng, H, K, kind, freqs[u % len(freqs)]) for u, kind in enumerate(("uniform5", "uniform400", "peaked"))]
    scan = np.concatenate([[0.0], np.linspace(1e-3, 0.5, n - 1)])          # F = 0, then the envelope's range 1e-3 .. 0.5
    grids = [np.roll(scan, 7 * u) for u in range(3)]
    rows = [u % len(freqs) for u in range(3)]
    got = run(H, K, tables, grids, rows, freqs)
    assert got.shape == (3, n)
    worst = 0.0
    for u in range(3):
        for i, F in enumerate(grids[u]):
            ok, err = ref.within(got[u][i], ref.evidence(tables[u], H, K, float(F), freqs[rows[u]]), float(F))
            worst = max(worst, err)
            assert ok, (u, i, F, got[u][i])
    print("600 grid points at H = 2, K = 2: worst |deviation| %.3g" % worst)
    # every point is what the same F gives alone
    for u, i in ((0, 0), (1, 300), (2, 545), (2, 546), (0, 599)):
        alone = run(H, K, [tables[u]], [[grids[u][i]]], [rows[u]], freqs)
        assert alone[0][0] == got[u][i], (u, i)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_an_all_zero_table_has_evidence_zero(name):
    """The priors are normalised: |evidence| <= FLOOR at every grid point, for every frequency variant of the case."""
    H, K, freqs, units = case_units(name)
    G = comb(H + K - 1, K)
    rows = list(range(len(freqs)))
    grids = [GRID7[u % 7:] + GRID7[:u % 7] for u in rows]
    got = run(H, K, [np.zeros(G)] * len(rows), grids, rows, freqs)
    worst = 0.0
    for u in rows:
        for n, F in enumerate(grids[u]):
            worst = max(worst, abs(got[u][n]))
            assert abs(got[u][n]) <= ref.floor(F), (name, u, F, got[u][n])
    flat = run(H, K, [np.zeros(G)], None)
    assert abs(flat[0][0]) <= ref.floor(None)
    print("%s: largest |evidence| of an all-zero table %.3g" % (name, worst))


SHIFT = -123.456


@pytest.mark.parametrize("name", ["cut-run", "first-of-KM16"])
def test_a_constant_added_to_a_table_is_added_to_every_evidence(name):
    H, K, freqs, units = case_units(name)
    base = run_case(name, "seven")
    grids = [grid_of("seven", u, None) for u in range(len(units))]
    moved = run(H, K, [llk + SHIFT for llk, _, _ in units], grids, [rec for _, rec, _ in units], freqs)
    for u in range(len(units)):
        for n, F in enumerate(grids[u]):
            ok, err = ref.within(moved[u][n], base[u][n] + SHIFT, F)
            assert ok, (name, u, F, moved[u][n], base[u][n], err)


def test_a_unit_without_a_finite_genotype_and_its_neighbours():
    name = "K4-H17"   # two tiles
    H, K, freqs, units = case_units(name)
    masked = [i for i, f in enumerate(freqs) if f[0] == 0.0][0]          # the record whose reference allele is masked
    from tests.estimate_reference import genotype_table

    holds_ref = np.any(genotype_table(H, K) == 0, axis=1)
    dead = [np.full(len(holds_ref), -np.inf),                             # no finite likelihood at all
            np.where(holds_ref, -1.0, -np.inf)]                           # finite only where the prior is -inf
    tables = [units[0][0], dead[0], units[1][0], dead[1], units[2][0]]
    rows = [units[0][1], masked, units[1][1], masked, units[2][1]]
    grids = [GRID3[i % 3] for i in range(5)]
    got = run(H, K, tables, grids, rows, freqs)
    assert np.all(got[[1, 3]] == -np.inf), got
    alone = run(H, K, [tables[i] for i in (0, 2, 4)], [grids[i] for i in (0, 2, 4)], [rows[i] for i in (0, 2, 4)], freqs)
    assert np.all(np.isfinite(alone)) and got[[0, 2, 4]].tobytes() == alone.tobytes()
    flat = run(H, K, [dead[0], dead[1]], None)
    assert flat[0][0] == -np.inf and np.isfinite(flat[1][0])              # (the flat prior knows no frequencies)


@pytest.mark.parametrize("name", ["tail-of-90", "K10-H7"])
def test_unit_order_and_a_second_build_give_equal_bits(name):
    H, K, freqs, units = case_units(name)
    base = run_case(name, "seven")
    assert run_case(name, "seven").tobytes() == base.tobytes()
    order = np.random.default_rng(5).permutation(len(units))
    assert not np.array_equal(order, np.arange(len(units)))
    shuffled = run_case(name, "seven", order)
    ok, _ = check(name, "seven", shuffled, order)
    assert ok and shuffled.tobytes() == base[order].tobytes()


def test_padded_frequency_rows_and_unit_row_indirection():
    name = "cut-run"
    H, K, freqs, units = case_units(name)
    base = run_case(name, "three")
    stride = H + 5
    place = [4, 0, 2]                                                     # the records' rows in a table of six padded rows
    assert len(freqs) == 3
    padded = np.full((6, stride), 0.25)                                   # (what a kernel reading a wrong row or past H would pick up)
    for i, p in enumerate(place):
        padded[p, :H] = freqs[i]
    grids = [grid_of("three", u, None) for u in range(len(units))]
    got = run(H, K, [llk for llk, _, _ in units], grids, [place[rec] for _, rec, _ in units], padded)
    assert got.tobytes() == base.tobytes()


def test_the_posteriors_of_the_shipped_caller():
    """For the configured prior exp(llk + log prior - evidence) sums to 1 and is ExactDeviceBatch.run(arrays=True)'s posterior
    array within that path's tolerance, and at the mode the streaming form's float64 probability within 1e-9 relative (the
    tolerances of tests/test_gpu_exact.py)."""
    from mchap_amd import calling
    from mchap_amd.device import ExactDeviceBatch
    from tests.estimate_reference import genotype_table
    from tests.estimate_units import make_record

    H, M, K = 6, 3, 4
    rng = np.random.default_rng(41)
    f = cases.frequency_row(rng, H, "no_zeros")
    unit = make_record(rng, H, M, (K, K, K), (14, 9, 11), f0=f)
    samples = list(unit["reads"])
    Fs = [0.0, 0.1, 0.5]
    R = max(len(unit["reads"][s]["counts"]) for s in samples)
    reads, counts = np.full((3, R, M, 2), np.nan), np.zeros((3, R), dtype=np.int64)
    for i, s in enumerate(samples):
        n = len(unit["reads"][s]["counts"])
        reads[i, :n], counts[i, :n] = unit["reads"][s]["dists"], unit["reads"][s]["counts"]
    batch = ExactDeviceBatch(reads, K, unit["locus"].haplotypes, counts, (np.array(Fs), unit["locus"].frequencies))
    batch.run(streaming=True, arrays=True, llks64=True)
    post = batch.array_results(True)["posteriors"]
    mode = batch.mode_results()
    llk = batch.out["llks64"].cpu().numpy().reshape(3, -1)
    got = run(H, K, list(llk), [(F,) for F in Fs], [0, 0, 0], np.stack([unit["locus"].frequencies]))
    g = genotype_table(H, K)
    for i, F in enumerate(Fs):
        mine = np.exp(llk[i] + ref.log_prior_lgamma(g, H, K, F, unit["locus"].frequencies) - got[i][0])
        print("F = %g: evidence %.9f, sum of exp(llk + log prior - evidence) - 1 = %.3g" % (F, got[i][0], mine.sum() - 1.0))
        assert abs(mine.sum() - 1.0) <= 1e-9
        # (the array path forms its posteriors from the float32 likelihoods, as the reference does: its tolerance in
        # tests/test_gpu_exact.py is max(3e-5, 4 float32 ulp of the largest |llk|) relative and 1e-12 absolute)
        ulp = float(np.spacing(np.float32(np.abs(llk[i]).max())))
        np.testing.assert_allclose(mine, post[i], rtol=max(3e-5, 4 * ulp), atol=1e-12)
        np.testing.assert_allclose(mine[calling.genotype_alleles_as_index(mode[0][i])], mode[2][i], rtol=1e-9)


# ---- the refusals of the entry: they return at the checks, before anything is launched (every buffer is nevertheless of the size
# a launch would read) ----
def _call(H, K, n_grid, stride=None, short=0, null=None, flat=False):
    import torch

    from mchap_amd import _lib

    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    stride = H if stride is None else stride
    G = comb(H + K - 1, K) if K <= 15 and comb(H + K - 1, K) < 1 << 24 else 16
    need = max(int(L.mchap_exact_evidence_workspace_bytes(1, H, K, max(n_grid, 1))), 256)
    t = dict(llk=torch.zeros(G, dtype=torch.float64, device=dev), F=torch.zeros(max(n_grid, 1), dtype=torch.float64, device=dev),
             row=torch.zeros(1, dtype=torch.int32, device=dev), f=torch.full((max(stride, H),), 1.0 / H, dtype=torch.float64, device=dev),
             ev=torch.full((max(n_grid, 1),), 7.0, dtype=torch.float64, device=dev), ws=torch.empty(need, dtype=torch.uint8, device=dev))
    p = lambda k: None if (k == null or (flat and k in ("F", "row", "f"))) else C.c_void_p(t[k].data_ptr())
    rc = L.mchap_exact_evidence_device(1, p("llk"), H, K, n_grid, p("F"), p("row"), p("f"), stride, p("ev"), p("ws"),
                                       C.c_int64(need - short), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, _lib.last_error(), t["ev"].cpu().numpy()


def test_refusals_at_the_entry():
    from mchap_amd import _lib

    untouched = lambda ev: np.all(ev == 7.0)
    for null in ("llk", "ev", "row", "f"):
        rc, msg, ev = _call(5, 2, 1, null=null)
        assert rc == _lib.ERR_BAD_ARG and "NULL buffer" in msg and untouched(ev), (null, msg)
    rc, msg, ev = _call(5, 2, 1, null="ws")
    assert rc == _lib.ERR_BAD_ARG and "too small" in msg and untouched(ev)
    rc, msg, ev = _call(5, 2, 1, stride=4)
    assert rc == _lib.ERR_BAD_ARG and "rows of 4 doubles for 5 haplotypes" in msg and untouched(ev)
    rc, msg, ev = _call(5, 2, 0)
    assert rc == _lib.ERR_BAD_ARG and "n_grid = 0" in msg and untouched(ev)
    rc, msg, ev = _call(5, 2, 3, flat=True)
    assert rc == _lib.ERR_BAD_ARG and "flat prior has one grid point" in msg and untouched(ev)
    rc, msg, ev = _call(5, 2, 3, short=1)
    assert rc == _lib.ERR_BAD_ARG and "too small" in msg and untouched(ev)
    rc, msg, ev = _call(5, _lib.MAX_PLOIDY_GENERAL + 1, 1)
    assert rc == _lib.ERR_LIMIT and "ploidy 16 not in 1..15" in msg and untouched(ev)
    assert comb(200 + 15 - 1, 15) >= 1 << 62 and int(_lib.lib().mchap_exact_evidence_workspace_bytes(1, 200, 15, 1)) == -1
    rc, msg, ev = _call(200, 15, 1)
    assert rc == _lib.ERR_LIMIT and "more than 2^62 genotypes" in msg and untouched(ev)
    # K = 2: 4 H + 4364 doubles of LDS for one table; H = 4030 is the first beyond 160 KB
    assert ev_lds_bytes(4029, 2, 1) <= 160 * 1024 < ev_lds_bytes(4030, 2, 1)
    assert int(_lib.lib().mchap_exact_evidence_chunk(4029, 2, 1)) == 1 and int(_lib.lib().mchap_exact_evidence_chunk(4030, 2, 1)) == 0
    rc, msg, ev = _call(4030, 2, 1)
    assert rc == _lib.ERR_LIMIT and "too large for the model evidence" in msg and untouched(ev)
    # and the same call with everything in place is taken: flat likelihoods under any normalised prior give 0; the flat prior too
    rc, msg, ev = _call(5, 2, 3)
    assert rc == _lib.OK and np.all(np.abs(ev) <= ref.floor(0.0)), (msg, ev)
    rc, msg, ev = _call(5, 2, 1, flat=True)
    assert rc == _lib.OK and abs(ev[0]) <= ref.floor(None), (msg, ev)


def test_inbreeding_outside_the_unit_interval_is_refused_on_the_host_copy():
    """The grid is checked where the caller's copy is on the host (device.ExactModelEvidence), before any launch."""
    import torch

    from mchap_amd.device import ExactModelEvidence

    ev = ExactModelEvidence()
    llks = torch.zeros(15, dtype=torch.float64, device=ev.device)
    for bad in (1.0, -1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            ev.add_group(llks, 5, 2, [[0.1, bad]], [0], np.full((1, 5), 0.2))
    with pytest.raises(ValueError, match="n_grid"):
        ev.add_group(llks, 5, 2, np.zeros((1, 0)), [0], np.full((1, 5), 0.2))
    with pytest.raises(NotImplementedError):
        ev.add_group(llks, 200, 15, [[0.1]], [0], np.full((1, 200), 0.005))
    assert ev.launches == 0
