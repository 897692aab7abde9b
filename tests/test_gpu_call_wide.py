"""GPU: `mchap call`'s sampler over many known haplotypes (call_wide_kernel behind CallingMCMC for more than 256 haplotypes, or
for any number under MCHAP_HIP_CALL_WIDE=1).

Up to 256 haplotypes the path is forced and held to the oracle on the same Philox streams -- alleles bit-exact step for step, llks
to 1e-10 -- and to the default path's traces.  Beyond 256, where the kernel runs in production, the same on the default dispatch
(the oracle's option arrays are sized by the haplotypes, and tests/test_call_wide.py holds it to the reference there): the
smallest shapes at which a round of 64 lanes, a key, a table row or the workgroup's LDS carve can go wrong.  Then determinism
(status, sorted alleles, no dependence on the batch or on the chains per workgroup), the stationary distribution against the
enumeration of all genotypes, the keys' rank arithmetic against exact integers, and the program `mchap call` on a haplotype VCF
with a record of 300 alternate alleles."""
import io as _io
import math
import os

import numpy as np
import pytest

from oracle import binding as orc
from tests.call_wide_helpers import largest_haps_below_2_62, many_haplotypes, rank_cases, wide_vcf

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
DEEP = ["simple.sample1.deep.bam", "simple.sample2.deep.bam", "simple.sample3.deep.bam"]


def _inputs(U, K, H, M, R, seed, qual=(5, 25), n_alleles=None):
    """the inputs of tests/test_gpu_call_mcmc.py (same shapes, same seeds)"""
    from mchap_amd.synth import synth_units

    rng = np.random.default_rng(seed)
    if n_alleles is not None:
        from tests.helpers import multiallelic_units

        reads, haps = multiallelic_units(rng, U, K, H, n_alleles, R, qual=qual, window=(2, M))
        return reads, haps, rng.integers(1, 4, size=(U, R)).astype(np.int64), rng
    reads, _, truth = synth_units(U, ploidy=K, n_pos=M, n_reads=R, first_unit=seed, window=(2, M), qual=qual)
    haps = np.zeros((U, H, M), np.int8)
    for u in range(U):
        pool = np.unique(np.concatenate([truth[u], rng.integers(0, 2, size=(6 * H, M)).astype(np.int8)]), axis=0)
        rng.shuffle(pool)
        haps[u] = pool[:H]
    counts = rng.integers(1, 4, size=(U, R)).astype(np.int64)
    return reads, haps, counts, rng


def _both_paths(monkeypatch, model, *args, **kw):
    monkeypatch.delenv("MCHAP_HIP_CALL_WIDE", raising=False)
    default = model.fit_batch(*args, **kw)
    monkeypatch.setenv("MCHAP_HIP_CALL_WIDE", "1")
    wide = model.fit_batch(*args, **kw)
    monkeypatch.delenv("MCHAP_HIP_CALL_WIDE", raising=False)
    return default, wide


# ---- 1. the wide path forced at up to 256 haplotypes: the oracle's traces and the default path's ----
@pytest.mark.parametrize("step_type", ["Gibbs", "Metropolis-Hastings"])
@pytest.mark.parametrize("K,H,M,R,na", [(4, 6, 6, 40, None), (2, 9, 5, 20, None), (6, 5, 4, 70, None), (3, 12, 6, 130, None),
                                        (4, 18, 6, 1400, None),
                                        (10, 6, 6, 50, None), (12, 5, 5, 90, None), (15, 4, 6, 40, None), (9, 7, 100, 60, None),
                                        (4, 8, 5, 60, [3] * 5), (6, 9, 6, 80, [2, 3, 4, 2, 4, 3]), (10, 6, 5, 50, [3, 2, 3, 3, 2]),
                                        (3, 256, 10, 40, None), (10, 12, 6, 50, None)],
                         ids=["K4", "K2", "K6", "K3", "deep", "K10", "K12", "K15", "K9-100snvs", "K4-A3", "K6-A4", "K10-A3", "H256", "K10-H12"])
def test_forced_wide_traces_match_oracle_and_default_path(step_type, K, H, M, R, na, monkeypatch):
    """The shapes of test_gpu_call_mcmc.py::test_traces_match_oracle_step_for_step, one of 256 haplotypes and one more of ploidy 10:
    both step types, with and without a prior, with and without read counts."""
    from mchap_amd.calling_mcmc import CallingMCMC

    U = 3
    reads, haps, counts, rng = _inputs(U, K, H, M, R, seed=K * 100 + H, n_alleles=na)
    F = np.array([0.0, 0.12, 0.3])
    fr = rng.dirichlet(np.ones(H), size=U)
    st = 0 if step_type == "Gibbs" else 1
    for prior, rc in ((None, None), (None, counts), ((F, None), counts), ((F, fr), counts), ((F, fr), None)):
        model = CallingMCMC(ploidy=K, haplotypes=haps[0], prior=None, steps=80, chains=2, random_seed=17, step_type=step_type)
        default, wide = _both_paths(monkeypatch, model, reads, rc, haplotypes=haps, prior=prior)
        for u in range(U):
            pr = None if prior is None else (float(F[u]), None if prior[1] is None else fr[u])
            g, l = orc.call_mcmc(reads[u], haps[u], K, steps=80, chains=2, step_type=st, read_counts=None if rc is None else rc[u],
                                 prior=pr, rng_kind=orc.RNG_PHILOX, seed=17, stream_id=u)
            assert np.array_equal(wide[u].genotypes, g), (u, prior is None, rc is None)
            np.testing.assert_allclose(wide[u].llks, l, rtol=1e-10, atol=1e-9)
            assert np.array_equal(wide[u].genotypes, default[u].genotypes), (u, prior is None, rc is None)
            assert wide[u].n_allele == H


@pytest.mark.parametrize("shape", ["settled", "wandering", "octoploid", "many-haplotypes"])
def test_forced_wide_on_the_memo_shapes(shape, monkeypatch):
    """The four shapes of test_gpu_call_mcmc.py::test_settled_chains_a_lane_each_give_the_same_traces: where the default path
    uses its Gibbs memo and hands settled chains over, this path does neither -- the same traces."""
    from mchap_amd.calling_mcmc import CallingMCMC

    K, H, M, R, qual, steps = {"settled": (4, 16, 8, 200, (5, 25), 400), "wandering": (4, 8, 6, 12, (2, 8), 700),
                               "octoploid": (8, 6, 5, 60, (5, 25), 300), "many-haplotypes": (3, 40, 8, 30, (3, 12), 300)}[shape]
    U = 5
    reads, haps, counts, rng = _inputs(U, K, H, M, R, seed=7 * K + H, qual=qual)
    model = CallingMCMC(ploidy=K, haplotypes=haps[0], prior=None, steps=steps, chains=3, random_seed=23)
    default, wide = _both_paths(monkeypatch, model, reads, None, haplotypes=haps, prior=(np.full(U, 0.1), None))
    for u in range(U):
        g, l = orc.call_mcmc(reads[u], haps[u], K, steps=steps, chains=3, step_type=0, prior=(0.1, None), rng_kind=orc.RNG_PHILOX, seed=23, stream_id=u)
        assert np.array_equal(wide[u].genotypes, g), u
        np.testing.assert_allclose(wide[u].llks, l, rtol=1e-10, atol=1e-9)
        assert np.array_equal(wide[u].genotypes, default[u].genotypes), u


# ---- 2. beyond 256: traces against the oracle on the default dispatch ----
CALL_WIDE_LDS = 160 * 1024 - 1024  # call_wide_kernel.hpp: the dynamic LDS a workgroup may ask for, four arrays [H] of doubles a chain


def _wg_chains(H, chains):
    """mchap_call_wide_wg_chains restated (it is not exported): the chains of a unit that share a workgroup"""
    wgc = min(chains, 4)
    while wgc > 1 and wgc * 4 * H * 8 > CALL_WIDE_LDS:
        wgc -= 1
    return wgc


def _wide_inputs(U, K, H, M, n_alleles=None):
    if n_alleles is None:
        return many_haplotypes(U, K, H, M, 12, seed=H + K, qual=(2, 8))
    from tests.helpers import multiallelic_units

    return multiallelic_units(np.random.default_rng(H + K), U, K, H, n_alleles, 12, qual=(2, 8), window=(2, len(n_alleles)))


def _against_oracle(K, H, reads, haps, steps, chains, step_type, prior, counts, initial=None, seed=17):
    """fit_batch on the default dispatch against orc.call_mcmc, unit by unit; returns the ORACLE's traces [U, chains, steps, K]"""
    from mchap_amd.calling_mcmc import CallingMCMC

    U = len(reads)
    model = CallingMCMC(ploidy=K, haplotypes=haps[0], prior=None, steps=steps, chains=chains, random_seed=seed, step_type=step_type)
    got = model.fit_batch(reads, counts, initial, haplotypes=haps, prior=prior)
    want = []
    for u in range(U):
        pr = None if prior is None else (float(prior[0][u]), None if prior[1] is None else prior[1][u])
        g, l = orc.call_mcmc(reads[u], haps[u], K, steps=steps, chains=chains, step_type=0 if step_type == "Gibbs" else 1,
                             read_counts=None if counts is None else counts[u], prior=pr, initial=None if initial is None else initial[u],
                             rng_kind=orc.RNG_PHILOX, seed=seed, stream_id=u)
        assert np.array_equal(got[u].genotypes, g), (u, step_type, prior is None, counts is None)
        np.testing.assert_allclose(got[u].llks, l, rtol=1e-10, atol=1e-9)
        assert got[u].n_allele == H
        want.append(g)
    return np.array(want)


def _moves(g):
    return int((g[:, :, 1:] != g[:, :, :-1]).any(axis=-1).sum())


WIDE_SHAPES = {  # K, H, M, steps, n_alleles
    "H257": (4, 257, 10, 40, None),            # one lane in the fifth round
    "H320": (3, 320, 10, 40, None),            # an exact multiple of 64
    "H321": (3, 321, 10, 40, None),            # one lane past it
    "H300": (4, 300, 10, 40, None),            # a partial last round
    "H1024": (4, 1024, 12, 40, None),          # many rounds
    "K7-H1024": (7, 1024, 12, 20, None),       # 2^57.7 genotypes
    "K8-H806": (8, 806, 12, 20, None),         # the 2^62 bound itself
    "H1273": (2, 1273, 12, 40, None),          # fewer than four chains fit a workgroup
    "H4096": (2, 4096, 13, 12, None),          # one chain per workgroup
    "K10-H300": (10, 300, 10, 20, None),       # the second instantiation, 2^60.7 genotypes
    "A3-A4": (4, 300, 6, 40, [3, 4, 2, 3, 4, 3]),  # reads of three and four alleles per SNV
}


@pytest.mark.parametrize("step_type", ["Gibbs", "Metropolis-Hastings"])
@pytest.mark.parametrize("shape", list(WIDE_SHAPES))
def test_wide_traces_match_oracle_beyond_256(shape, step_type, monkeypatch):
    """call_wide_kernel where it runs in production against the oracle: 2 units of distinct haplotype sets (3 chains; 2 at K >= 7 or
    H >= 1024, 4 at H = 1273), without a
    prior and counts, with (F, None) and with (F, freqs) and counts (F = 0, 0.12: F = 0 has its own branch), and once from a given
    initial genotype.  The case is worth its name only if the ORACLE's chains move and visit alleles above 255: asserted."""
    from mchap_amd import _lib

    K, H, M, steps, na = WIDE_SHAPES[shape]
    # (4 chains at H = 1273: three share a workgroup and the fourth runs alone; 2 where the oracle's own time is the test's)
    U, chains = 2, 4 if shape == "H1273" else 2 if (K >= 7 or H >= 1024) else 3
    monkeypatch.delenv("MCHAP_HIP_CALL_WIDE", raising=False)
    monkeypatch.delenv("MCHAP_HIP_CALL_WIDE_CHAINS", raising=False)
    assert H > 256 and H <= int(_lib.lib().mchap_call_mcmc_max_haps(K))
    if shape == "H4096":
        assert H == int(_lib.lib().mchap_call_mcmc_max_haps(2))
    if shape == "K8-H806":
        assert H == largest_haps_below_2_62(8)
    assert _wg_chains(H, chains) == {"H1273": 3, "H4096": 1}.get(shape, chains)  # (H1273: fewer than its four chains; H4096: one)
    reads, haps = _wide_inputs(U, K, H, M, na)
    rng = np.random.default_rng(K * 1000 + H)
    counts = rng.integers(1, 4, size=reads.shape[:2]).astype(np.int64)
    F = np.array([0.0, 0.12, 0.3])[:U]
    fr = rng.dirichlet(np.ones(H), size=U)
    recorded = U * chains * (steps - 1)
    moves, beyond = 0, 0
    runs = [(prior, rc, None) for prior, rc in ((None, None), ((F, None), counts), ((F, fr), counts))]
    runs.append(((F, fr), counts, np.sort(np.concatenate([rng.integers(0, H, size=(U, K - 1)), np.full((U, 1), H - 1)], axis=1), axis=1).astype(np.int64)))
    for prior, rc, initial in runs:
        g = _against_oracle(K, H, reads, haps, steps, chains, step_type, prior, rc, initial=initial)
        assert (np.diff(g, axis=-1) >= 0).all() and g.max() < H
        print("%s %s prior %s initial %s: %d moves of %d recorded steps, %d alleles above 255"
              % (shape, step_type, prior is not None and (prior[1] is None and "F" or "F, freqs"), initial is not None, _moves(g), recorded, int((g > 255).sum())))
        if step_type == "Gibbs":  # every run of the case: at least half of its recorded steps change genotype
            assert 2 * _moves(g) >= recorded, (shape, _moves(g), recorded)
        moves += _moves(g)
        beyond += int((g > 255).sum())
    assert beyond > 0, shape
    assert moves >= 2, (shape, moves)  # (Metropolis-Hastings: at least twice per case)


def test_wide_chains_over_more_than_one_workgroup(monkeypatch):
    """K = 4 over 300 haplotypes with 1, 4, 5 and 9 chains (5 and 9: a unit's chains in more than one workgroup, the last one
    partly filled), and again with one chain per workgroup: the oracle's traces each time."""
    K, H, M, steps, U = 4, 300, 10, 40, 2
    reads, haps = _wide_inputs(U, K, H, M)
    prior = (np.array([0.0, 0.12]), None)
    monkeypatch.delenv("MCHAP_HIP_CALL_WIDE", raising=False)
    for forced in (None, "1"):
        if forced is None:
            monkeypatch.delenv("MCHAP_HIP_CALL_WIDE_CHAINS", raising=False)
        else:
            monkeypatch.setenv("MCHAP_HIP_CALL_WIDE_CHAINS", forced)
        for chains in (1, 4, 5, 9):
            for step_type in ("Gibbs", "Metropolis-Hastings"):
                g = _against_oracle(K, H, reads, haps, steps, chains, step_type, prior, None)
                assert (g > 255).any() and _moves(g) >= (2 if step_type != "Gibbs" else (U * chains * (steps - 1)) // 2)
    monkeypatch.delenv("MCHAP_HIP_CALL_WIDE_CHAINS", raising=False)


def test_one_haplotype_past_the_genotype_bound_is_refused_by_name():
    from mchap_amd.calling_mcmc import CallingMCMC

    H = largest_haps_below_2_62(8) + 1
    assert H == 807
    reads, haps = many_haplotypes(1, 8, H, 12, 8, seed=3)
    with pytest.raises(NotImplementedError, match="2\\^62"):
        CallingMCMC(ploidy=8, haplotypes=haps[0], steps=10, chains=1, random_seed=1).fit(reads[0])


# ---- 3. the keys' rank arithmetic on the device ----
# the lowest top allele (0-based) from which cwr's product r * (n - 1 + d) passes 2^63 at a shape the 2^62 rule admits
CWR_OVERFLOWS_FROM = {11: 205, 12: 159, 13: 128, 14: 107, 15: 92}


def _device_keys(g, which):
    """mchap_debug_call_keys (the parity suite's library): which = 0 / 1 call_key<8> / <16>, 2 / 3 call_wide_key<8> / <16>"""
    import ctypes as C

    from mchap_amd import _lib

    os.environ["MCHAP_HIP_TEST_KERNELS"] = "1"
    try:
        L = _lib.lib()
        f = L.mchap_debug_call_keys
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        g32 = np.ascontiguousarray(g, dtype=np.int32)
        out = np.full(len(g32), -1, np.int64)
        rc = f(g32.ctypes.data, len(g32), g32.shape[1], which, out.ctypes.data)
        assert rc == 0, L.mchap_last_error().decode()
    finally:
        os.environ.pop("MCHAP_HIP_TEST_KERNELS", None)
    return out


@pytest.mark.parametrize("K", range(2, 16))
def test_device_keys_are_the_exact_ranks(K):
    """call_key (call_mcmc_kernel, up to 256 haplotypes) and call_wide_key (call_wide_kernel, up to 4096) on the device against exact
    Python integers: the genotypes of tests/test_call_wide.py's rank test at the largest shape each kernel and the 2^62 rule admit,
    and at ploidies 11 to 15 genotypes whose top allele is at or above the point where the product-before-division form overflows.
    Integers: no tolerance."""
    rng = np.random.default_rng(K)
    km = 0 if K <= 8 else 1
    for which, top in ((km, 256), (2 + km, 4096)):
        H = min(top, largest_haps_below_2_62(K))
        # (the largest shape is (806, 8), (105, 15), ... itself, and (4096, 5) on the wide key; two more shapes of the CPU test lie below it)
        sets = [rank_cases(K, H)] + [rank_cases(K, h) for h in {7: [1024], 10: [300]}.get(K, []) if h <= H]
        if K in CWR_OVERFLOWS_FROM:
            lo = CWR_OVERFLOWS_FROM[K]
            assert lo < H
            g = np.sort(np.concatenate([rng.integers(0, H, size=(200, K - 1)), rng.integers(lo, H, size=(200, 1))], axis=1), axis=1)
            g = np.concatenate([g, np.sort(rng.integers(lo, H, size=(100, K)), axis=1), [np.append(np.zeros(K - 1, np.int64), lo)]])
            sets.append((g, [sum(math.comb(int(a) + i, i + 1) for i, a in enumerate(row)) for row in g]))
        for g, exact in sets:
            assert max(exact) < 1 << 62
            shuffled = rng.permuted(g, axis=1)  # (the keys sort their alleles themselves)
            got = _device_keys(shuffled, which)
            bad = [i for i in range(len(g)) if int(got[i]) != exact[i]]
            assert not bad, (which, H, len(bad), g[bad[0]].tolist(), int(got[bad[0]]), exact[bad[0]])


def test_device_summaries_of_wide_traces_equal_the_host_classes():
    """test_gpu_call_mcmc.py::test_device_summaries_of_call_traces_equal_the_host_classes over 300 haplotypes at ploidy 4, what the
    program reads off call_wide_kernel's traces: two units of 3 poor reads (900 steps x 3 chains: more than 512 distinct genotypes,
    the listed launch) and a settled unit of 200 good reads in one batch (the poor units' reads padded with all-NaN rows, which
    add nothing to a likelihood).  Every assertion of that test but the GP array: as_array(300) at ploidy 4 is
    C(303, 4) = 3.4e8 doubles."""
    from mchap_amd.calling_mcmc import CallingMCMC

    K, H, M, steps, chains, R = 4, 300, 10, 900, 3, 200
    poor, haps_p = many_haplotypes(2, K, H, M, 3, seed=41, qual=(2, 6))
    good, haps_g = many_haplotypes(1, K, H, M, R, seed=43)
    reads = np.full((3, R) + poor.shape[2:], np.nan)
    reads[:2, :3] = poor
    reads[2] = good[0]
    haps = np.concatenate([haps_p, haps_g])
    U, burn = 3, steps // 3
    model = CallingMCMC(ploidy=K, haplotypes=haps[0], prior=None, steps=steps, chains=chains, random_seed=29)
    kw = dict(haplotypes=haps, prior=(np.full(U, 0.15), None))
    got = model.fit_batch_summaries(reads, None, burn=burn, incongruence_threshold=0.6, **kw)
    traces = model.fit_batch(reads, None, **kw)
    sizes = []
    for u in range(U):
        tr = traces[u].burn(burn)
        post = tr.posterior()
        assert np.array_equal(got[u].genotypes, post.genotypes), u
        np.testing.assert_array_equal(got[u].counts / got[u].n_obs, post.probabilities)
        alleles, gprob, sprob = post.mode(genotype_support=True)
        assert np.array_equal(got[u].alleles, alleles) and abs(got[u].gprob - gprob) < 1e-15 and abs(got[u].sprob - sprob) < 1e-12
        assert got[u].mci == tr.replicate_incongruence(threshold=0.6)
        for a, b in zip(got[u].posterior_frequencies(), tr.posterior_frequencies()):
            assert len(a) == H
            np.testing.assert_array_equal(a, b)
        labels = np.arange(H) * 2 + 1
        np.testing.assert_array_equal(got[u].relabel(labels).posterior_frequencies()[2], tr.relabel(labels).posterior_frequencies()[2])
        sizes.append(len(post.probabilities))
    print("distinct genotypes per unit:", sizes)
    assert max(sizes[:2]) > 512 and sizes[2] < 64, sizes
    assert (np.asarray(traces[0].genotypes) > 255).any()


# ---- 4. beyond 256: determinism, the stationary distribution, the program ----
@pytest.mark.parametrize("step_type", ["Gibbs", "Metropolis-Hastings"])
@pytest.mark.parametrize("H", [300, 1024])
def test_beyond_256_runs_and_is_deterministic(H, step_type, monkeypatch):
    """300 and 1024 known haplotypes at ploidy 4: status 0, every step's alleles sorted and below H, and a unit's trace depends
    neither on the other units of the batch nor on the number of chains a workgroup holds."""
    from mchap_amd import _lib
    from mchap_amd.calling_mcmc import CallingMCMC

    K, M, R, U, steps, chains = 4, 12, 40, 3, 40, 3
    assert int(_lib.lib().mchap_call_mcmc_max_haps(K)) >= 1024
    reads, haps = many_haplotypes(U, K, H, M, R, seed=H)
    model = CallingMCMC(ploidy=K, haplotypes=haps[0], prior=None, steps=steps, chains=chains, random_seed=5, step_type=step_type)
    prior = (np.full(U, 0.1), None)
    monkeypatch.delenv("MCHAP_HIP_CALL_WIDE_CHAINS", raising=False)
    traces = model.fit_batch(reads, None, haplotypes=haps, prior=prior)  # (raises on a non-zero status)
    for t in traces:
        g = np.asarray(t.genotypes)
        assert g.shape == (chains, steps, K) and (g >= 0).all() and (g < H).all() and (np.diff(g, axis=-1) >= 0).all()
        assert np.isfinite(t.llks).all() and t.n_allele == H
    # a unit on its own (its stream id kept) and in another order
    alone = model.fit_batch(reads[1:2], None, haplotypes=haps[1:2], prior=(prior[0][1:2], None), stream_ids=np.array([1], dtype=np.uint64))
    assert np.array_equal(alone[0].genotypes, traces[1].genotypes) and np.array_equal(alone[0].llks, traces[1].llks)
    back = model.fit_batch(reads[::-1], None, haplotypes=haps[::-1], prior=prior, stream_ids=np.arange(U, dtype=np.uint64)[::-1])
    for u in range(U):
        assert np.array_equal(back[U - 1 - u].genotypes, traces[u].genotypes) and np.array_equal(back[U - 1 - u].llks, traces[u].llks)
    # one chain per workgroup instead of as many as the LDS holds
    monkeypatch.setenv("MCHAP_HIP_CALL_WIDE_CHAINS", "1")
    single = model.fit_batch(reads, None, haplotypes=haps, prior=prior)
    for u in range(U):
        assert np.array_equal(single[u].genotypes, traces[u].genotypes) and np.array_equal(single[u].llks, traces[u].llks)


def test_beyond_the_bound_is_a_limit_by_name():
    from mchap_amd import _lib
    from mchap_amd.calling_mcmc import CallingMCMC

    top = int(_lib.lib().mchap_call_mcmc_max_haps(2))
    reads, haps = many_haplotypes(1, 2, top + 1, 14, 8, seed=1)
    with pytest.raises(NotImplementedError, match=str(top)):
        CallingMCMC(ploidy=2, haplotypes=haps[0], steps=10, chains=1, random_seed=1).fit(reads[0])
    # the genotype-count rule stays, by its own name (1024 haplotypes at ploidy 8: 2^64.7 genotypes)
    reads, haps = many_haplotypes(1, 8, 1024, 12, 8, seed=2)
    with pytest.raises(NotImplementedError, match="2\\^62"):
        CallingMCMC(ploidy=8, haplotypes=haps[0], steps=10, chains=1, random_seed=1).fit(reads[0])


def test_stationary_distribution_over_300_haplotypes():
    """300 known haplotypes at ploidy 2 (45 150 genotypes), 2 chains, burn 1000, both step types (as
    test_gpu_call_mcmc.py::test_gibbs_and_mh_agree_with_the_exact_posterior): the posterior allele frequencies of the trace
    against genotype_posteriors + posterior_allele_frequencies over all genotypes, within the project's 0.015.

    The run length is set by the reference's own sampler on this input (tests/golden/make_call_wide.py: its CallingMCMC under
    numpy's generator, 25 000 steps x 2 chains; the fixture records its distance from the enumeration per step type).
      Gibbs: 0.0007 at 25 000 steps -- within 0.015 with far more than a factor of two to spare: 25 000 steps.
      Metropolis-Hastings: 0.035 at 25 000 steps -- it MISSES 0.015 (one of 299 alleles proposed uniformly: few proposals are
      accepted).  A sampling error falls as 1 / sqrt(steps), so the reference meets 0.015 with a factor of two to spare
      (0.0075) at ceil((0.035 / 0.0075)^2) = 22 times the length: 550 000 steps, computed below from the fixture's figure.  The
      reference itself has not been run at that length (hours of interpreted Python); the length rests on the square-root law
      (single runs scatter around it: a reference run of 7 000 steps lay at 0.049)."""
    from math import ceil

    from mchap_amd import calling
    from mchap_amd.calling_mcmc import CallingMCMC

    z = np.load(os.path.join(os.path.dirname(HERE), "call_wide.npz"))
    reads, haps, K = z["reads"], z["haplotypes"], int(z["ploidy"])
    H = len(haps)
    steps, chains, burn = int(z["steps"]), int(z["chains"]), int(z["burn"])
    assert (K, H, steps, chains, burn) == (2, 300, 25000, 2, 1000)
    ref = {"Gibbs": float(z["ref_max_abs_diff"]), "Metropolis-Hastings": float(z["ref_mh_max_abs_diff"])}
    length = {st: steps * max(1, ceil((v / (0.015 / 2)) ** 2)) for st, v in ref.items()}
    assert length["Gibbs"] == steps and length["Metropolis-Hastings"] <= 40 * steps, (ref, length)
    llks = calling.genotype_likelihoods(reads, K, haps).astype(np.float64)
    exact = calling.posterior_allele_frequencies(calling.genotype_posteriors(llks, K, H, None), K, H)[0]
    np.testing.assert_allclose(exact, z["ref_exact_freqs"], rtol=0, atol=1e-4)  # (the fixture is this input: the reference's enumeration)
    for step_type in ("Gibbs", "Metropolis-Hastings"):
        trace = CallingMCMC(ploidy=K, haplotypes=haps, prior=None, steps=length[step_type], chains=chains, random_seed=11, step_type=step_type).fit(reads)
        got = trace.burn(burn).posterior_frequencies()[0]
        diff = float(np.abs(got - exact).max())
        print("%s, %d steps: max |d freq| = %.5f (reference sampler at %d steps: %.5f)" % (step_type, length[step_type], diff, steps, ref[step_type]))
        assert diff < 0.015, step_type


def test_call_program_calls_a_record_of_300_alternate_alleles(tmp_path, capfd):
    """`mchap call` on a haplotype VCF with a record of 300 ALT alleles among the ordinary ones: every record is called, none is
    LIMIT, the neighbours' lines are those of a run without the wide record; a record beyond mchap_call_mcmc_max_haps is still a
    LIMIT record with its warning."""
    from mchap_amd import _lib, cli

    base = os.path.join(HERE, "simple.output.deep.assemble.vcf")
    top = int(_lib.lib().mchap_call_mcmc_max_haps(4))
    with_wide, with_both = str(tmp_path / "wide.vcf"), str(tmp_path / "both.vcf")
    wide_vcf(base, with_wide, [("CHR1", 6, "WIDE300", 300)])
    wide_vcf(base, with_both, [("CHR1", 6, "WIDE300", 300), ("CHR2", 11, "BEYOND", top + 1)])

    def run(vcf):
        out = _io.StringIO()
        cli.run(["mchap_amd", "call", "--bam"] + [os.path.join(HERE, f) for f in DEEP] + ["--ploidy", "4", "--haplotypes", vcf,
                 "--mcmc-steps", "300", "--mcmc-burn", "100", "--mcmc-seed", "5", "--report", "AFP"], out)
        return [ln for ln in out.getvalue().splitlines() if ln and not ln.startswith("#")]

    plain, wide = run(base), run(with_wide)
    capfd.readouterr()
    assert len(wide) == len(plain) + 1
    rec = [ln.split("\t") for ln in wide]
    assert all(f[6] != "LIMIT" for f in rec)
    (w,) = [f for f in rec if f[2] == "WIDE300"]
    assert len(w[4].split(",")) == 300 and all("." not in s.split(":")[0] for s in w[9:])
    assert [ln for ln in wide if ln.split("\t")[2] != "WIDE300"] == plain
    both = run(with_both)
    err = capfd.readouterr().err
    by = {ln.split("\t")[2]: ln.split("\t") for ln in both}
    assert by["BEYOND"][6] == "LIMIT" and by["BEYOND"][9].split(":")[0] == "./././."
    assert "not called" in err and "FILTER=LIMIT" in err and str(top) in err
    assert [ln for ln in both if ln.split("\t")[2] != "BEYOND"] == wide
