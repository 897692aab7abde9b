"""The kernels of the identity evidence -- identity_prior_kernel<8|16>, identity_a_kernel, identity_product_kernel,
identity_combine_kernel -- driven through device.ExactIdentity on drawn likelihoods, against the float64 host definition
(application.identity_unit; tests/test_identity_reference.py holds it to long double on the CPU).  The bound on a term:
|got - want| <= 1e-9 |want| + (G + 4096) 2^-52 (tests/identity_reference.py); -inf, NaN and the exact 0 must match exactly.  Every
launch holds 3 records; record 0 is under a zero frequency and holds two rows peaked 2000 nats apart on different genotypes (the
clause), record 1 a sample without reads, record 2 a sample whose likelihoods are all -inf.  Samples: 1 (one cell), 3 (less than
a tile), 17 and 33 (of the issue's list), 65 (across the edge of the kernel's tile of 64).  Largest |device - host| over the
suite, measured on an MI355X: see DESIGN.md 4.4."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

from tests import identity_reference as ref

pytestmark = pytest.mark.gpu

TILE = 64   # the kernel's tile of samples (exact_identity_kernel.hpp IDENTITY_TILE)
SAMPLES = (1, 3, 17, 33, TILE + 1)
CASES = [(K, H, n) for K, H in ref.SHAPES for n in SAMPLES]


@functools.lru_cache(maxsize=None)
def case(K, H, n):
    return ref.draw_case(K, H, n)


@functools.lru_cache(maxsize=None)
def host(K, H, n, F, e):
    """float64 [3, n, n]: the host definition of every record."""
    from mchap_amd import application

    llk, reads, fr = case(K, H, n)
    return np.stack([application.identity_unit(llk[r], ref.log_prior(K, H, F, fr[r]), e, reads[r]) for r in range(len(llk))])


def device(K, H, llk, reads, fr, F, e, rows=None):
    """The evidence launch for log Z, then one identity launch -> lbf [R, n, n] on the host."""
    import torch

    from mchap_amd.device import ExactIdentity, ExactModelEvidence

    dev = ExactIdentity()
    R, n, G = llk.shape
    rows = np.arange(R) if rows is None else np.asarray(rows)
    d_llk = torch.from_numpy(np.ascontiguousarray(llk, dtype=np.float64)).to(dev.device).reshape(-1)
    grid = None if F is None else np.full((R * n, 1), F)
    norm = ExactModelEvidence(dev.device).add_group(d_llk, H, K, grid, np.repeat(rows, n), fr).reshape(R, n).contiguous()
    got = dev.log_bayes_factors(d_llk, H, K, F, rows, fr, norm, e, reads)
    torch.cuda.synchronize()
    assert dev.launches == 1
    return got.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("K, H, n", CASES, ids=["K%d-H%d-n%d" % c for c in CASES])
def test_against_the_host_definition(K, H, n):
    llk, reads, fr = case(K, H, n)
    G = llk.shape[2]
    worst = 0.0
    for F in ref.PRIORS:
        for e in (0.0, 0.01):
            got = device(K, H, llk, reads, fr, F, e)
            want = host(K, H, n, F, e)
            ok, err = ref.within(got, want, G)
            worst = max(worst, err if np.isfinite(err) else worst)
            assert ok, (K, H, n, F, e, err)
            assert np.array_equal(bits(got), bits(np.swapaxes(got, 1, 2)))          # got[r][i][j] and got[r][j][i], every cell
            assert all(np.all(np.isnan(np.diag(got[r]))) for r in range(3))
            if n >= 2:
                # the clause: the two peaked rows of record 0
                assert got[0, 0, n - 1] == (-np.inf if e == 0.0 else np.log(0.01))
            if n >= 3:
                off = [i for i in range(n) if i != 2]
                assert np.all(got[1, 1, [j for j in range(n) if j != 1 and not (n >= 17 and j == 5)]] == 0.0)   # the sample without reads
                assert np.all(np.isnan(got[2, 2])) and np.all(np.isfinite(got[2][np.ix_(off, off)][~np.eye(n - 1, dtype=bool)]))
            if n >= 17:
                assert np.isnan(got[1, 1, 5]) and np.isnan(got[1, 5, 1])              # no finite genotype beside no reads
    print("K=%d H=%d (G=%d) n=%d: largest |device - host| of a term %.3g (bound's floor %.3g)" % (K, H, G, n, worst, ref.floor(G)))


def test_equal_bits_whatever_the_place_and_the_company():
    K, H, n, F, e = 4, 16, 33, 0.3, 0.01
    llk, reads, fr = case(K, H, n)
    first = device(K, H, llk, reads, fr, F, e)
    assert np.array_equal(bits(first), bits(device(K, H, llk, reads, fr, F, e)))                                # twice over
    assert np.array_equal(bits(first[::-1]), bits(device(K, H, llk[::-1], reads[::-1], fr[::-1], F, e)))        # reversed records
    p = np.random.default_rng(5).permutation(n)
    assert np.array_equal(bits(first[:, p][:, :, p]), bits(device(K, H, llk[:, p], reads[:, p], fr, F, e)))     # both axes alike
    # a pair alone, one record, against its cell
    for r, i, j in ((0, 3, 20), (0, 0, 32), (1, 7, 11), (2, 30, 4), (1, 1, 8)):
        alone = device(K, H, llk[r:r + 1, [i, j]], reads[r:r + 1, [i, j]], fr[r:r + 1], F, e)
        assert bits(alone)[0, 0, 1] == bits(first)[r, i, j] and bits(alone)[0, 1, 0] == bits(first)[r, j, i]
    # ... and across the edge of a tile, under the flat prior at e = 0
    llk, reads, fr = case(6, 6, TILE + 1)
    first = device(6, 6, llk, reads, fr, None, 0.0)
    for r, i, j in ((0, 3, 64), (2, 64, 63)):
        alone = device(6, 6, llk[r:r + 1, [i, j]], reads[r:r + 1, [i, j]], fr[r:r + 1], None, 0.0)
        assert bits(alone)[0, 0, 1] == bits(first)[r, i, j]


def test_a_workspace_one_byte_short_and_the_refused_shapes():
    import torch

    from mchap_amd import _lib
    from mchap_amd.device import ExactIdentity, ExactModelEvidence, _ptr

    L = _lib.lib()
    wb = ExactIdentity.workspace_bytes
    assert wb(1, 2, 4, 16) == -1 and wb(1, 2, 4, 0) == -1            # a ploidy outside 1..15
    assert wb(1, 2, 100000, 15) == -1                                # 2^62 genotypes
    assert wb(0, 2, 4, 4) == 0 and wb(1, 1, 4, 4) > 0
    K, H, n = 4, 4, 3
    llk, reads, fr = case(K, H, n)
    G = llk.shape[2]
    need = wb(3, n, H, K)
    assert need >= 3 * n * G * 8
    dev = ExactIdentity()
    d_llk = torch.from_numpy(llk).to(dev.device).reshape(-1)
    norm = ExactModelEvidence(dev.device).add_group(d_llk, H, K, None, None, None).reshape(3, n).contiguous()
    out = torch.empty((3, n, n), dtype=torch.float64, device=dev.device)
    ws = torch.empty(need, dtype=torch.uint8, device=dev.device)
    d_reads = torch.from_numpy(reads).to(dev.device)

    def call(offered, ploidy=K, error=0.01):
        return L.mchap_exact_identity_device(3, n, _ptr(d_llk), H, ploidy, None, None, 0, _ptr(norm), C.c_double(error), _ptr(d_reads),
                                             _ptr(out), 3, _ptr(ws), C.c_int64(offered), None)

    assert call(need - 1) == _lib.ERR_LIMIT and call(need, 16) == _lib.ERR_LIMIT
    assert call(need, K, 1.5) == _lib.ERR_BAD_ARG
    assert call(need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(device(K, H, llk, reads, fr, None, 0.01)))
    with pytest.raises(NotImplementedError):
        dev.log_bayes_factors(d_llk, H, K, None, None, None, norm, 0.01, reads, workspace_limit=need - 1)
    for bad in (1.5, -1e-9, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            dev.log_bayes_factors(d_llk, H, K, None, None, None, norm, bad, reads)
    # prior tables beyond the LDS: refused with a prior, as the evidence launch refuses the shape
    assert int(L.mchap_exact_evidence_chunk(20000, 1, 1)) == 0
    big = torch.zeros(2 * 20000, dtype=torch.float64, device=dev.device)
    with pytest.raises(NotImplementedError):
        dev.log_bayes_factors(big, 20000, 1, 0.1, [0], np.full((1, 20000), 1.0 / 20000), torch.zeros((1, 2), dtype=torch.float64, device=dev.device), 0.01)


def test_the_calling_layer_takes_numpy_in_and_gives_numpy_out():
    from mchap_amd import application, calling

    K, H, n = 4, 4, 3
    llk, reads, fr = case(K, H, n)
    got = calling.identity_log_bayes_factors(llk[0], None, 0.01)
    assert isinstance(got, np.ndarray) and got.shape == (n, n)
    assert np.array_equal(bits(got), bits(device(K, H, llk[:1], None, fr[:1], None, 0.01)[0]))
    lp = ref.log_prior(K, H, 0.3, fr[1])
    rows = llk[2, [0, 1]]
    got = calling.identity_log_bayes_factors(rows, lp, 0.0)
    ok, err = ref.within(got, application.identity_unit(rows, lp, 0.0), llk.shape[2])
    assert ok, err
