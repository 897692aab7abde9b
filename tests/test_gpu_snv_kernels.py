"""The kernels of the SNV genotype posteriors -- exact_snv_kernel<8|16>, exact_snv_combine_kernel, after the evidence launches for
the normaliser -- driven through device.ExactSnvPosteriors with the synthetic likelihood tables of tests/estimate_cases.py, against
the long-double reference (tests/snv_posterior_reference.py; tests/test_snv_posterior_reference.py anchors it on the CPU): every
case with M = 5 under the units' own F (F = 0 and F > 0 mixed in a launch) and under the flat prior, the SNVs worked in chunks, the
rows' layout, a unit without a finite genotype, unit order, equal bits, the properties that need no reference, and the entry's
refusals."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

from tests import estimate_cases as cases
from tests import snv_posterior_reference as ref

pytestmark = pytest.mark.gpu

M = 5


def snv_lds_bytes(H, K, S, chunk):
    """exact_snv_lds (exact_kernel.hpp), restated: the prior tables of one F, the chunk's SNV alleles as bytes (rounded up to 8),
    and one region that is first the staging tile and then the chunk's bins."""
    return (H * (K + 1) + (K + 1) + H + 1) * 8 + ((H * chunk + 7) & ~7) + max(256 * 17 * 8, chunk * S * 8)


def snv_chunk(H, K, n_pos, A):
    """exact_snv_chunk, restated: SNVs per chunk within 64 KB, at least one (up to 160 KB), 0 beyond."""
    S = comb(A + K - 1, K)
    if snv_lds_bytes(H, K, S, 1) > 160 * 1024:
        return 0
    c = 1
    while c < n_pos and snv_lds_bytes(H, K, S, c + 1) <= 64 * 1024:
        c += 1
    return c


@functools.lru_cache(maxsize=None)
def case_units(name):
    """(H, K, freqs [records, H], units [(llk, record, own F)], hap_alleles int8 [records, H, M]) of a case: every record its own
    SNV alleles."""
    K, H, _ = cases.CASES[name]
    records = cases.build_case(name)
    ha = np.stack([ref.case_hap_alleles("%s-%d" % (name, i), H, M) for i in range(len(records))])
    return H, K, np.stack([r["f"] for r in records]), [(llk, i, F) for i, r in enumerate(records) for llk, _, F in r["units"]], ha


@functools.lru_cache(maxsize=None)
def reference(name, flat):
    """[U] of float64 [M, S]: the long-double posteriors of a case, computed once."""
    H, K, freqs, units, ha = case_units(name)
    S = comb(int(ha.max()) + K, K)
    out = [ref.snv_posteriors(llk, H, K, None if flat else F, freqs[rec], ha[rec], S) for llk, rec, F in units]
    for a in out:
        a.setflags(write=False)
    return out


def run(H, K, tables, Fs, rows, freqs, ha, with_norm=False):
    """device.ExactSnvPosteriors.add_group over `tables` -> float64 [U, M, S] on the host."""
    import torch

    from mchap_amd.device import ExactSnvPosteriors

    snv = ExactSnvPosteriors()
    llks = torch.from_numpy(np.concatenate(tables)).to(snv.device)
    got = snv.add_group(llks, H, K, Fs, rows, freqs, ha)
    torch.cuda.synchronize()
    return (got.cpu().numpy(), snv.log_norm.cpu().numpy()) if with_norm else got.cpu().numpy()


def run_case(name, flat=False, order=None):
    H, K, freqs, units, ha = case_units(name)
    order = list(range(len(units))) if order is None else list(order)
    return run(H, K, [units[u][0] for u in order], None if flat else [units[u][2] for u in order], [units[u][1] for u in order], freqs, ha)


def check(name, flat, got, order=None):
    H, K, freqs, units, ha = case_units(name)
    want = reference(name, flat)
    order = list(range(len(units))) if order is None else list(order)
    ok, worst = True, 0.0
    for i, u in enumerate(order):
        o, err = ref.within(got[i], want[u], comb(H + K - 1, K))
        ok, worst = ok and o, max(worst, err)
    return ok, worst


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_kernels_against_long_double(name):
    H, K, freqs, units, ha = case_units(name)
    G = comb(H + K - 1, K)
    Fs = [F for _, _, F in units]
    assert 0.0 in Fs and any(F > 0 for F in Fs)   # F = 0 and F > 0 in one launch
    for flat in (False, True):
        got = run_case(name, flat)
        assert got.shape == (len(units), M, comb(int(ha.max()) + K, K))
        ok, worst = check(name, flat, got)
        print("%s, %s: worst |deviation| %.3g (REL %g, FLOOR %.3g)" % (name, "flat prior" if flat else "own F", worst, ref.REL, ref.floor(G)))
        assert ok, (name, flat, worst)
        # rows sum to 1, the entries beyond an SNV's own genotypes are exactly 0, a monomorphic SNV is 1 at rank 0
        assert np.all(np.abs(got.sum(axis=2) - 1.0) <= ref.floor(G) * got.shape[2])
        for u, (_, rec, _) in enumerate(units):
            for j in range(M):
                assert np.all(got[u, j, comb(int(ha[rec, :, j].max()) + K, K):] == 0.0)
            assert abs(got[u, 0, 0] - 1.0) <= ref.floor(G)


def test_the_snvs_are_worked_in_chunks_where_the_bins_do_not_fit():
    from mchap_amd import _lib

    L = _lib.lib()
    for K, H, _ in cases.CASES.values():
        for n, A in ((1, 1), (5, 2), (5, 4), (12, 4), (40, 3)):
            assert int(L.mchap_exact_snv_chunk(H, K, n, A)) == snv_chunk(H, K, n, A), (K, H, n, A)
    assert int(L.mchap_exact_snv_chunk(5, 2, 5, 5)) == 0 and int(L.mchap_exact_snv_chunk(5, 16, 5, 2)) == 0
    # K = 2: 4 H + 4 doubles of tables, H bytes of alleles, the 34 816-byte tile; H = 3909 is the first beyond 160 KB
    assert snv_lds_bytes(3908, 2, 3, 1) <= 160 * 1024 < snv_lds_bytes(3909, 2, 3, 1)
    assert int(L.mchap_exact_snv_chunk(3908, 2, 5, 2)) == 1 and int(L.mchap_exact_snv_chunk(3909, 2, 5, 2)) == 0
    name, n = "K15-H6", 12
    K, H, _ = cases.CASES[name]
    S = comb(4 + K - 1, K)
    assert S == 816 and n * S * 8 > 64 * 1024
    chunk = snv_chunk(H, K, n, 4)
    assert 1 < chunk < n and n % chunk != 0   # several chunks, the last one partial
    _, _, freqs, units, _ = case_units(name)
    ha = np.stack([ref.case_hap_alleles("chunks-%d" % i, H, n) for i in range(len(freqs))])
    ha[:, :4, n - 1] = np.arange(4)           # four alleles in the last, partial chunk too
    assert int(ha.max()) == 3
    args = ([llk for llk, _, _ in units], [F for _, _, F in units], [rec for _, rec, _ in units], freqs)
    got = run(H, K, *args, ha)
    assert got.shape == (len(units), n, S)
    worst = 0.0
    for u, (llk, rec, F) in enumerate(units):
        ok, err = ref.within(got[u], ref.snv_posteriors(llk, H, K, F, freqs[rec], ha[rec], S), comb(H + K - 1, K))
        worst = max(worst, err)
        assert ok, (u, err)
    print("K15-H6, 12 SNVs in chunks of %d: worst |deviation| %.3g" % (chunk, worst))
    for j in (0, 1, chunk - 1, chunk, n - 1):   # every SNV's row is what the SNV gives as a launch of its own
        alone = run(H, K, *args, np.ascontiguousarray(ha[:, :, j:j + 1]))
        width = alone.shape[2]
        assert alone[:, 0, :].tobytes() == np.ascontiguousarray(got[:, j, :width]).tobytes(), j
        assert np.all(got[:, j, width:] == 0.0)


def test_padded_rows_and_unit_row_indirection():
    name = "cut-run"
    H, K, freqs, units, ha = case_units(name)
    base = run_case(name)
    stride = H + 5
    place = [4, 0, 2]                                                     # the records' rows in tables of six rows
    assert len(freqs) == 3 and int(ha.max()) == 3
    padded = np.full((6, stride), 0.25)                                   # (what a kernel reading a wrong row or past H would pick up)
    alleles = np.full((6, H, M), 3, dtype=np.int8)
    for i, p in enumerate(place):
        padded[p, :H] = freqs[i]
        alleles[p] = ha[i]
    got = run(H, K, [llk for llk, _, _ in units], [F for _, _, F in units], [place[rec] for _, rec, _ in units], padded, alleles)
    assert got.tobytes() == base.tobytes()


def test_a_unit_without_a_finite_genotype_and_its_neighbours():
    name = "K4-H17"   # two tiles
    H, K, freqs, units, ha = case_units(name)
    masked = [i for i, f in enumerate(freqs) if f[0] == 0.0][0]          # the record whose reference allele is masked
    from tests.estimate_reference import genotype_table

    holds_ref = np.any(genotype_table(H, K) == 0, axis=1)
    dead = [np.full(len(holds_ref), -np.inf),                             # no finite likelihood at all
            np.where(holds_ref, -1.0, -np.inf)]                           # finite only where the prior is -inf
    tables = [units[0][0], dead[0], units[1][0], dead[1], units[2][0]]
    rows = [units[0][1], masked, units[1][1], masked, units[2][1]]
    Fs = [units[0][2], 0.1, units[1][2], 0.0, units[2][2]]
    got, norm = run(H, K, tables, Fs, rows, freqs, ha, with_norm=True)
    assert np.all(np.isnan(got[[1, 3]])) and np.all(norm[[1, 3]] == -np.inf)
    keep = [0, 2, 4]
    alone = run(H, K, [tables[i] for i in keep], [Fs[i] for i in keep], [rows[i] for i in keep], freqs, ha)
    assert not np.any(np.isnan(alone)) and got[keep].tobytes() == alone.tobytes()
    flat = run(H, K, dead, None, [masked, masked], freqs, ha)
    assert np.all(np.isnan(flat[0])) and not np.any(np.isnan(flat[1]))   # (the flat prior knows no frequencies)


@pytest.mark.parametrize("name", ["tail-of-90", "K10-H7"])
def test_unit_order_and_a_second_run_give_equal_bits(name):
    H, K, freqs, units, ha = case_units(name)
    base = run_case(name)
    assert run_case(name).tobytes() == base.tobytes()
    order = np.random.default_rng(5).permutation(len(units))
    assert not np.array_equal(order, np.arange(len(units)))
    shuffled = run_case(name, order=order)
    ok, _ = check(name, False, shuffled, order)
    assert ok and shuffled.tobytes() == base[order].tobytes()


def test_distinct_alleles_give_the_haplotype_posterior():
    """M = 1, K = 4, H = 4 with four distinct SNV alleles: snv_post[0] is exp(llk + log prior - log_norm), element for element."""
    from mchap_amd.application import _genotype_table, _host_log_prior

    H = K = 4
    G = comb(H + K - 1, K)
    rng = np.random.default_rng(11)
    f = cases.frequency_row(rng, H, "no_zeros")
    tables = [cases.likelihood_table(rng, H, K, kind, f) for kind in ("uniform5", "uniform400", "holes")]
    Fs = [0.0, 0.1, 0.5]
    ha = np.arange(4, dtype=np.int8).reshape(1, 4, 1)
    for flat in (False, True):
        got, norm = run(H, K, tables, None if flat else Fs, [0, 0, 0], np.stack([f]), ha, with_norm=True)
        assert got.shape == (3, 1, G)
        for u in range(3):
            with np.errstate(invalid="ignore"):
                want = np.exp(tables[u] + _host_log_prior(_genotype_table(H, K), H, K, None if flat else Fs[u], f) - norm[u])
            assert np.all(np.abs(got[u, 0] - want) <= ref.REL * want + ref.floor(G)), (flat, u)
            assert ref.within(got[u], ref.snv_posteriors(tables[u], H, K, None if flat else Fs[u], f, ha[0]), G)[0]


def test_the_expected_dosages_are_the_streaming_form_s_frequencies():
    """K x ExactDeviceBatch.mode_results' freqs, added up by SNV allele, against the dosages of snv_post: 1e-9 relative."""
    from mchap_amd.application import _genotype_table
    from mchap_amd.device import ExactDeviceBatch, ExactSnvPosteriors
    from tests.estimate_units import make_record

    import torch

    H, Mr, K = 6, 3, 4
    rng = np.random.default_rng(41)
    f = cases.frequency_row(rng, H, "no_zeros")
    unit = make_record(rng, H, Mr, (K, K, K), (14, 9, 0), f0=f)   # (the third sample has no reads: its posterior is its prior)
    samples = list(unit["reads"])
    Fs = [0.0, 0.1, 0.5]
    R = max(1, max(len(unit["reads"][s]["counts"]) for s in samples))
    reads, counts = np.full((3, R, Mr, 2), np.nan), np.zeros((3, R), dtype=np.int64)
    for i, s in enumerate(samples):
        n = len(unit["reads"][s]["counts"])
        reads[i, :n], counts[i, :n] = unit["reads"][s]["dists"], unit["reads"][s]["counts"]
    haps = unit["locus"].haplotypes
    batch = ExactDeviceBatch(reads, K, haps, counts, (np.array(Fs), f))
    batch.run(streaming=True)
    llks = batch.run_llks64()
    got = ExactSnvPosteriors().add_group(llks, H, K, Fs, [0, 0, 0], np.stack([f]), haps[None])
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    freqs = batch.mode_results()[4]
    table = _genotype_table(2, K)[:got.shape[2]]
    alt_copies = (table == 1).sum(axis=1)
    for u in range(3):
        for j in range(Mr):
            want = K * freqs[u][haps[:, j] == 1].sum()
            assert abs(got[u, j] @ alt_copies - want) <= 1e-9 * want + ref.floor(comb(H + K - 1, K)), (u, j)
    assert np.all(np.abs(got.sum(axis=2) - 1.0) <= ref.floor(comb(H + K - 1, K)) * got.shape[2])


# ---- the refusals of the entry: they return at the checks, before anything is launched (every buffer is nevertheless of the size
# a launch would read) ----
def _call(H, K, n_pos=2, A=2, stride=None, short=0, null=None, flat=False):
    import torch

    from mchap_amd import _lib

    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    stride = H if stride is None else stride
    small = 1 <= K <= 15 and comb(H + K - 1, K) < 1 << 24
    G = comb(H + K - 1, K) if small else 16
    S = comb(A + K - 1, K) if small and 1 <= A <= 4 else 16
    need = max(int(L.mchap_exact_snv_workspace_bytes(1, H, K, max(n_pos, 1), A)), 256)
    t = dict(llk=torch.zeros(G, dtype=torch.float64, device=dev), F=torch.zeros(1, dtype=torch.float64, device=dev),
             row=torch.zeros(1, dtype=torch.int32, device=dev), f=torch.full((max(stride, H),), 1.0 / H, dtype=torch.float64, device=dev),
             ha=torch.zeros(H * max(n_pos, 1), dtype=torch.int8, device=dev),
             out=torch.full((max(n_pos, 1) * S,), 7.0, dtype=torch.float64, device=dev), norm=torch.full((1,), 7.0, dtype=torch.float64, device=dev),
             ws=torch.empty(need, dtype=torch.uint8, device=dev))
    p = lambda k: None if (k == null or (flat and k in ("F", "f"))) else C.c_void_p(t[k].data_ptr())
    rc = L.mchap_exact_snv_posteriors_device(1, p("llk"), H, K, n_pos, A, p("F"), p("row"), p("f"), stride, p("ha"), p("out"), p("norm"),
                                             p("ws"), C.c_int64(need - short), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, _lib.last_error(), np.concatenate([t["out"].cpu().numpy(), t["norm"].cpu().numpy()])


def test_refusals_at_the_entry():
    from mchap_amd import _lib

    L = _lib.lib()
    untouched = lambda out: np.all(out == 7.0)
    for null in ("llk", "out", "row", "ha", "f"):
        rc, msg, out = _call(5, 2, null=null)
        assert rc == _lib.ERR_BAD_ARG and "NULL buffer" in msg and untouched(out), (null, msg)
    rc, msg, out = _call(5, 2, null="ws")
    assert rc == _lib.ERR_BAD_ARG and "too small" in msg and untouched(out)
    rc, msg, out = _call(5, 2, short=1)
    assert rc == _lib.ERR_BAD_ARG and "too small" in msg and untouched(out)
    rc, msg, out = _call(5, 2, stride=4)
    assert rc == _lib.ERR_BAD_ARG and "rows of 4 doubles for 5 haplotypes" in msg and untouched(out)
    for A in (0, 5):
        rc, msg, out = _call(5, 2, A=A)
        assert rc == _lib.ERR_BAD_ARG and "n_snv_alleles = %d not in 1..4" % A in msg and untouched(out)
    rc, msg, out = _call(5, 2, n_pos=0)
    assert rc == _lib.ERR_BAD_ARG and "n_pos = 0" in msg and untouched(out)
    for K in (0, _lib.MAX_PLOIDY_GENERAL + 1):
        assert int(L.mchap_exact_snv_workspace_bytes(1, 5, K, 2, 2)) == -1
        rc, msg, out = _call(5, K)
        assert rc == _lib.ERR_LIMIT and "ploidy %d not in 1..15" % K in msg and untouched(out)
    assert comb(200 + 15 - 1, 15) >= 1 << 62 and int(L.mchap_exact_snv_workspace_bytes(1, 200, 15, 2, 2)) == -1
    rc, msg, out = _call(200, 15)
    assert rc == _lib.ERR_LIMIT and "more than 2^62 genotypes" in msg and untouched(out)
    rc, msg, out = _call(3909, 2)
    assert rc == _lib.ERR_LIMIT and "too large for the SNV posteriors" in msg and untouched(out)
    # and the same call with everything in place is taken: every haplotype carries allele 0, so rank 0 holds everything; log_norm of
    # an all-zero table under a normalised prior is 0
    for flat in (False, True):
        rc, msg, out = _call(5, 2, flat=flat)
        post, norm = out[:-1].reshape(2, 3), out[-1]
        assert rc == _lib.OK and abs(norm) <= ref.floor(15), (msg, out)
        assert np.all(np.abs(post[:, 0] - 1.0) <= ref.floor(15)) and np.all(post[:, 1:] == 0.0)


def test_the_host_copies_are_checked_before_any_launch():
    import torch

    from mchap_amd.device import ExactSnvPosteriors

    snv = ExactSnvPosteriors()
    llks = torch.zeros(15, dtype=torch.float64, device=snv.device)
    ha = np.zeros((1, 5, 2), dtype=np.int8)
    for bad in (1.0, -1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            snv.add_group(llks, 5, 2, [bad], [0], np.full((1, 5), 0.2), ha)
    for bad in (4, -1):
        with pytest.raises(ValueError, match="SNV allele"):
            snv.add_group(llks, 5, 2, [0.1], [0], np.full((1, 5), 0.2), np.full((1, 5, 2), bad, dtype=np.int8))
    with pytest.raises(NotImplementedError):
        snv.add_group(llks, 200, 15, [0.1], [0], np.full((1, 200), 0.005), np.zeros((1, 200, 2), dtype=np.int8))
    assert snv.launches == 0
