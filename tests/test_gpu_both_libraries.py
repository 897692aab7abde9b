"""libmchap_hip.so and libmchap_hip_test.so link the same exact-caller and call-sampler objects: the same small batch through one
and then the other in one process gives bit-equal outputs, and the oracle's (compared as tests/test_gpu_exact.py and
tests/test_gpu_call_mcmc.py compare them)."""
import numpy as np
import pytest

from oracle import binding as orc

pytestmark = pytest.mark.gpu

U, R, M, H, K = 2, 8, 3, 4, 2
STEPS, CHAINS, SEED = 50, 2, 17


def _units():
    from mchap_amd.synth import synth_units

    rng = np.random.default_rng(20)
    reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, first_unit=20, window=(2, M), qual=(5, 25))
    haps = np.zeros((U, H, M), np.int8)
    for u in range(U):
        pool = np.unique(rng.integers(0, 2, size=(8 * H, M)).astype(np.int8), axis=0)
        rng.shuffle(pool)
        assert len(pool) >= H
        haps[u] = pool[:H]
    counts = rng.integers(1, 4, size=(U, R)).astype(np.int64)
    return reads, haps, counts


def _run(reads, haps, counts, prior):
    from mchap_amd import calling
    from mchap_amd.calling_mcmc import CallingMCMC

    mode = calling.posterior_mode_batch(reads, K, haps, counts, prior, True, True, True)
    traces = CallingMCMC(ploidy=K, haplotypes=haps[0], prior=None, steps=STEPS, chains=CHAINS, random_seed=SEED).fit_batch(
        reads, counts, haplotypes=haps, prior=prior)
    return [np.array(x) for x in mode], [(t.genotypes.copy(), t.llks.copy()) for t in traces]


def test_exact_caller_and_call_sampler_are_the_same_objects_in_both_libraries(monkeypatch):
    reads, haps, counts = _units()
    assert reads.shape == (U, R, M, 2)
    F = np.array([0.1, 0.3])
    prior = (F, None)
    monkeypatch.delenv("MCHAP_HIP_TEST_KERNELS", raising=False)
    mode_a, traces_a = _run(reads, haps, counts, prior)
    monkeypatch.setenv("MCHAP_HIP_TEST_KERNELS", "1")
    mode_b, traces_b = _run(reads, haps, counts, prior)
    # bit-equal between the libraries
    assert len(mode_a) == len(mode_b) == 6
    for a, b in zip(mode_a, mode_b):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for (ga, la), (gb, lb) in zip(traces_a, traces_b):
        assert ga.tobytes() == gb.tobytes() and la.tobytes() == lb.tobytes()
    # ... and the oracle's
    for u in range(U):
        pr = (float(F[u]), None)
        a, ml, mp, sp, fq, oc = orc.posterior_mode(reads[u], K, haps[u], counts[u], pr)
        assert mode_a[0][u].tolist() == a.tolist()
        np.testing.assert_allclose([mode_a[1][u], mode_a[2][u], mode_a[3][u]], [ml, mp, sp], rtol=1e-9)
        np.testing.assert_allclose(mode_a[4][u], fq, rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(mode_a[5][u], oc, rtol=1e-9, atol=1e-300)
        g, l = orc.call_mcmc(reads[u], haps[u], K, steps=STEPS, chains=CHAINS, step_type=0, read_counts=counts[u], prior=pr,
                             rng_kind=orc.RNG_PHILOX, seed=SEED, stream_id=u)
        assert traces_a[u][0].shape == (CHAINS, STEPS, K)
        assert np.array_equal(traces_a[u][0], g)
        np.testing.assert_allclose(traces_a[u][1], l, rtol=1e-10, atol=1e-9)
