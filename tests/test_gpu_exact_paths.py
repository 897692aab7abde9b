"""The exact caller's kernel paths one by one against the oracle.  The host picks, per launch, an untiled or a tiled product
table, the KM = 8 or KM = 16 instantiation, the grouped-logarithm loop (every read weight 1) or the weighted per-read sum
(and the per-read loop for the R % 4 last reads), the cached or the plain second pass, and reduces the mode over blocks of 4096
genotypes; reads carry 2 to 4 alleles per position.  Each case below names the path it covers and asserts that the host's rule
(restated in tests/fuzz_exact.py) does send it there, so that a change of a threshold fails here instead of leaving a path
untested.  Every output of both forms is checked by fuzz_exact.check_exact_batch (tolerances of tests/test_gpu_exact.py)."""
import ctypes as C
import os
import sys
from math import comb

import numpy as np
import pytest

from oracle import binding as orc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fuzz_exact import check_exact_batch, exact_path  # noqa: E402
from tests.helpers import multiallelic_units  # noqa: E402

BI6 = [2] * 6
TRI = [2, 3, 2, 3, 3, 2]
TETRA = [2, 3, 4, 2, 4, 3]


def _counts(kind, rng, U, R):
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones((U, R), np.int64)
    if kind == "one-two":  # all ones but a single weight of 2: the weighted loop
        c = np.ones((U, R), np.int64)
        c[:, R // 2] = 2
        return c
    return rng.integers(1, 4, size=(U, R)).astype(np.int64)


def _prior(kind, rng, U, H):
    F = np.array([0.1, 0.3, 0.0][:U])
    return {"none": None, "F": (F, None), "F+freqs": (F, rng.dirichlet(np.ones(H), size=U))}[kind]


def _assert_path(R, H, K, counts, tiled, km16, multi_block, w01):
    for u in range(1 if counts is None else len(counts)):
        p = exact_path(R, H, K, None if counts is None else counts[u])
        assert (p["tiled"], p["km16"], p["multi_block"], p["w01"]) == (tiled, km16, multi_block, w01), p


def _run(K, H, na, R, ckind, pkind, seed, tiled, km16, multi_block, U=2):
    rng = np.random.default_rng(seed)
    reads, haps = multiallelic_units(rng, U, K, H, na, R, window=(2, len(na)))
    counts = _counts(ckind, rng, U, R)
    _assert_path(R, H, K, counts, tiled, km16, multi_block, ckind in ("none", "ones"))
    assert reads.shape[-1] == max(na)
    check_exact_batch(reads, K, haps, counts, _prior(pkind, rng, U, H))


# ---- unweighted reads, untiled: every R % 4 tail of the grouped-logarithm loop ----
@pytest.mark.parametrize("ckind", ["none", "ones"])
@pytest.mark.parametrize("R", [1, 2, 3, 5, 203])
def test_unweighted_untiled_every_tail(R, ckind):
    _run(4, 8, BI6, R, ckind, "F+freqs", 10 + R, tiled=False, km16=False, multi_block=False)


# ---- unweighted / weighted, tiled (K4 over 24 haplotypes: 17 550 genotypes, 5 blocks) ----
@pytest.mark.parametrize("ckind", ["none", "ones", "one-two"])
@pytest.mark.parametrize("R", [1500, 1501])
def test_tiled_reads(R, ckind):
    _run(4, 24, BI6, R, ckind, "F+freqs", 20 + R, tiled=True, km16=False, multi_block=True)


# ---- KM = 16 over several genotype blocks ----
@pytest.mark.parametrize("pkind", ["none", "F", "F+freqs"])
@pytest.mark.parametrize("ckind", ["none", "1-3"])
@pytest.mark.parametrize("K,H", [(10, 8), (12, 6), (15, 6)], ids=["K10-H8", "K12-H6", "K15-H6"])
def test_high_ploidy_several_blocks(K, H, ckind, pkind):
    _run(K, H, BI6, 60, ckind, pkind, 30 + K, tiled=False, km16=True, multi_block=True)


# ---- KM = 16, tiled (K10 over 8 haplotypes, 2500 reads: 191 KB of products) ----
@pytest.mark.parametrize("ckind", ["none", "1-3"])
def test_high_ploidy_tiled(ckind):
    _run(10, 8, [2, 2, 2, 2, 2], 2500, ckind, "F+freqs", 40, tiled=True, km16=True, multi_block=True)


# ---- tri- and tetra-allelic SNVs (reads [R, M, A] of as_probabilistic, gaps included) ----
_MULTI = [(K, H, R, False, False, na, "K%d-%s" % (K, nm)) for K, H, R in ((2, 12, 80), (4, 10, 120), (6, 8, 90), (10, 6, 60))
          for na, nm in ((TRI, "A3"), (TETRA, "A4"))]
_MULTI += [(2, 30, 700, True, False, TRI, "K2-tiled-A3"), (4, 24, 1500, True, True, TETRA, "K4-tiled-A4"),
           (6, 12, 1600, True, True, TRI, "K6-tiled-A3"), (10, 8, 2500, True, True, TETRA, "K10-tiled-A4")]


@pytest.mark.parametrize("K,H,R,tiled,multi_block,na", [c[:6] for c in _MULTI], ids=[c[6] for c in _MULTI])
def test_multiallelic(K, H, R, tiled, multi_block, na):
    # (tiled: weighted reads only -- the unweighted tiled loop is test_tiled_reads' and test_high_ploidy_tiled's)
    for ckind in (("1-3",) if tiled else ("none", "1-3")):
        _run(K, H, na, R, ckind, "F+freqs", 50 + K + len(na) + H, tiled=tiled, km16=K > 8, multi_block=multi_block)


# ---- zero-weight padding as application._run_exact_groups builds it ----
@pytest.mark.parametrize("K,H,na,Rmax", [(4, 8, TETRA, 203), (4, 24, TRI, 1501), (10, 8, BI6, 90)], ids=["K4", "K4-tiled", "K10"])
def test_zero_weight_padding(K, H, na, Rmax):
    rng = np.random.default_rng(60 + K + H)
    lens = [Rmax, 0, 1, 37, Rmax - 2]
    U = len(lens)
    full, haps = multiallelic_units(rng, U, K, H, na, Rmax)
    reads = np.full(full.shape, np.nan)
    counts = np.zeros((U, Rmax), np.int64)
    oracle_inputs = []
    for u, n in enumerate(lens):
        c = rng.integers(1, 4, size=n).astype(np.int64) if u % 2 else np.ones(n, np.int64)
        reads[u, :n] = full[u, :n]
        counts[u, :n] = c
        oracle_inputs.append((full[u, :n], c))
    assert exact_path(Rmax, H, K, counts[0])["tiled"] == (Rmax > 1000)
    # (unit 0 fills the rows with weights 1: the grouped loop; the zero rows make every other unit weighted)
    assert [exact_path(Rmax, H, K, counts[u])["w01"] for u in range(U)] == [True] + [False] * (U - 1)
    F = rng.choice([0.0, 0.2], size=U)
    check_exact_batch(reads, K, haps, counts, (F, rng.dirichlet(np.ones(H), size=U)), oracle_inputs=oracle_inputs)


# ---- ties across genotype blocks: the first genotype in VCF order, as np.argmax ----
@pytest.mark.parametrize("K,H", [(4, 24), (10, 8)], ids=["K4", "K10"])
def test_no_information_ties_give_genotype_zero(K, H):
    """One all-gap read (the device entry refuses R = 0), no prior: every genotype has the same joint value, bit for bit."""
    rng = np.random.default_rng(70 + K)
    _, haps = multiallelic_units(rng, 2, K, H, BI6, 1)
    reads = np.full((2, 1, 6, 2), np.nan)
    _assert_path(1, H, K, None, tiled=False, km16=K > 8, multi_block=True, w01=True)
    batch = check_exact_batch(reads, K, haps, None, None, exact_ties=True)
    assert (batch.mode_results()[0] == 0).all() and (batch.array_results(False)["alleles"] == 0).all()


@pytest.mark.parametrize("K,H,a,b", [(4, 24, 16, 20), (10, 8, 6, 7)], ids=["K4", "K10"])
def test_prior_ties_across_blocks_give_the_first(K, H, a, b):
    """Haplotypes a < b are the same sequence and the reads come from a homozygote of it; under an inbreeding-only prior the two
    homozygotes a^K and b^K have the same joint value bit for bit and lie in different blocks: the mode is a^K in both forms."""
    from mchap_amd import calling
    from mchap_amd.encoding import as_probabilistic

    ia, ib = calling.genotype_alleles_as_index([a] * K), calling.genotype_alleles_as_index([b] * K)
    assert ia // 4096 != ib // 4096 and ia >= 4096
    rng = np.random.default_rng(80 + K)
    U, M, R = 2, 6, 40
    reads = np.empty((U, R, M, 2))
    haps = np.zeros((U, H, M), np.int8)
    for u in range(U):
        _, hp = multiallelic_units(rng, 1, K, H, BI6, 1)
        haps[u] = hp[0]
        haps[u, b] = haps[u, a]
        calls = np.broadcast_to(haps[u, a], (R, M)).copy()
        calls[rng.random((R, M)) < 0.2] = -1
        reads[u] = as_probabilistic(calls, 2, 0.99)
    _assert_path(R, H, K, None, tiled=False, km16=K > 8, multi_block=True, w01=True)
    batch = check_exact_batch(reads, K, haps, None, (np.array([0.2, 0.5]), None), exact_ties=True)
    assert (batch.mode_results()[0] == a).all() and (batch.array_results(False)["alleles"] == a).all()


# ---- mchap_exact_posterior_summaries_batch_device on posterior arrays of the oracle ----
def _summaries(post, K, H):
    import torch

    from mchap_amd import _lib

    U, G = post.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    d_post = torch.from_numpy(np.ascontiguousarray(post).reshape(-1)).to(dev)
    ma = torch.empty(U * K, dtype=torch.int64, device=dev)
    mp, sp = (torch.empty(U, dtype=torch.float64, device=dev) for _ in range(2))
    fr, cn, oc = (torch.empty(U * H, dtype=torch.float64, device=dev) for _ in range(3))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(_lib.lib().mchap_exact_posterior_summaries_batch_device(
        U, p(d_post), C.c_int64(G), K, H, p(ma), p(mp), p(sp), p(fr), p(cn), p(oc), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    h = lambda t, *s: t.cpu().numpy().reshape(s)  # noqa: E731
    return h(ma, U, K), h(mp, U), h(sp, U), h(fr, U, H), h(cn, U, H), h(oc, U, H)


@pytest.mark.parametrize("K,H", [(4, 20), (6, 12), (10, 8), (12, 6)], ids=["K4-H20", "K6-H12", "K10-H8", "K12-H6"])
def test_posterior_summaries_batch_device(K, H):
    from mchap_amd import calling

    rng = np.random.default_rng(90 + K)
    G = comb(H + K - 1, K)
    assert G > 4096
    reads, haps = multiallelic_units(rng, 2, K, H, TRI, 30)
    rows = []
    for u in range(2):
        e32, e64 = orc.genotype_likelihoods(reads[u], K, haps[u])
        rows.append(orc.genotype_posteriors(e64, K, H, (0.1, None)))
    rows.append(np.full(G, 1.0 / G))  # every genotype tied: index 0
    tie = rng.random(G)
    i1, i2 = 4096 + int(rng.integers(0, 100)), G - 1 - int(rng.integers(0, 100))
    tie[i1] = tie[i2] = 3.0   # the maximum twice, in different blocks: the first
    rows.append(tie / tie.sum())
    flat = np.zeros(G)
    flat[G // 2:] = 1.0 / (G - G // 2)  # a tie that starts inside a later block
    rows.append(flat)
    post = np.stack(rows)
    ma, mp, sp, fr, cn, oc = _summaries(post, K, H)
    for u, p in enumerate(post):
        idx = int(np.argmax(p))
        assert ma[u].tolist() == calling.index_as_genotype_alleles(idx, K).tolist(), (u, idx)
        assert mp[u] == p[idx]
        np.testing.assert_allclose(sp[u], calling.alternate_dosage_posteriors(ma[u], p)[1].sum(), rtol=1e-12)
        rf, rc, ro = orc.posterior_allele_frequencies(p, K, H)
        np.testing.assert_allclose(np.stack([fr[u], cn[u], oc[u]]), np.stack([rf, rc, ro]), rtol=1e-9, atol=1e-300)
    assert calling.genotype_alleles_as_index(ma[2]) == 0 and calling.genotype_alleles_as_index(ma[3]) == i1
    assert calling.genotype_alleles_as_index(ma[4]) == G // 2
