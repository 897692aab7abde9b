"""Differential soak of the exact caller (mchap_exact_call_batch_device: exact_pass1 / exact_mode / exact_pass2 / exact_freq /
exact_array kernels) against the oracle on random shapes: ploidy 1-15, 2-40 known haplotypes, 1-12 SNVs of 2-4 alleles each,
1-2600 reads, read counts absent / all ones / 1-4 / with zeros, no prior / inbreeding / inbreeding and frequencies.  Every
output of the streaming form (with and without the joint values cached between its passes) and of the array form is held to
the oracle (check_exact_batch, which tests/test_gpu_exact_paths.py uses as well).  Needs a GPU; uses the oracle, hence lives
under tests/.  python tests/fuzz_exact.py [cases] [seed]"""
import os
import sys
from math import comb

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ---- the host's choice of kernel path (mchap_amd/csrc/exact_api.hip, exact_kernel.hpp), restated ----
EXACT_THREADS = 256
EXACT_GENOS_PER_BLOCK = 4096


def exact_pass1_lds(R, H, K):
    return (R * H + R + H * (K + 1) + (K + 1) + H + 5 * EXACT_THREADS) * 8


def exact_rows(R, H, K):
    """Rows of the LDS product table: R when the untiled pass fits 160 KB, else the tile (a multiple of four reads)."""
    if exact_pass1_lds(R, H, K) <= 160 * 1024:
        return R
    fixed = exact_pass1_lds(0, H, K) + 64
    budget = 144 * 1024
    if fixed >= budget:
        return 0
    rows = ((budget - fixed) // ((H + 1) * 8)) & ~3
    return rows if rows >= 32 else 0


def exact_path(R, H, K, counts=None):
    """What the launch of one unit takes: tiled product table, the KM = 16 instantiation, several genotype blocks, the
    grouped-logarithm (every read weight 1) loop, and the R % 4 reads the per-read loop takes."""
    rows = exact_rows(R, H, K)
    G = comb(H + K - 1, K)
    return dict(G=G, rows=rows, tiled=0 < rows < R, km16=K > 8, nblk=-(-G // EXACT_GENOS_PER_BLOCK),
                multi_block=G > EXACT_GENOS_PER_BLOCK, w01=counts is None or bool(np.all(np.asarray(counts) == 1)), tail=R % 4)


def _log_prior(G, K, H, pr):
    from oracle import binding as orc

    with np.errstate(divide="ignore"):
        return np.log(orc.genotype_posteriors(np.zeros(G), K, H, pr))


def check_exact_batch(reads, K, haps, counts=None, prior=None, exact_ties=False, oracle_inputs=None):
    """Runs a batch through ExactDeviceBatch -- the streaming form with the joint values cached and without, the array form
    with float32 and float64 likelihoods -- and asserts every output against the oracle unit by unit (AssertionError).

    Tolerances as tests/test_gpu_exact.py: likelihoods float32 2.5e-7, float64 1e-10 relative; the streaming summaries 1e-9;
    the posterior array max(3e-5, 4 ulp of float32) relative.  The streaming mode's alleles equal the oracle's, except where the
    two genotypes' joint values (float64 llk + log prior) lie within 1e-12 relative of each other: which of two sums that
    differ in their last bits is the larger is not something two implementations agree on (tests/fuzz_call.py); then the
    device's genotype must be one of the tied ones and its statistics are those of that genotype.  exact_ties=True: no such
    exception (genotypes tied bit for bit: the first in VCF order, as np.argmax, in either form).  oracle_inputs: per unit
    (reads, counts) the oracle is given instead of the batch's (the zero-weight padding of application._run_exact_groups)."""
    from oracle import binding as orc

    from mchap_amd import calling
    from mchap_amd.device import ExactDeviceBatch

    reads = np.asarray(reads, dtype=np.float64)
    U, R, M, A = reads.shape
    H = haps.shape[1]
    G = comb(H + K - 1, K)
    batch = ExactDeviceBatch(reads, K, haps, counts, prior)
    batch.run(streaming=True, arrays=True, llks64=True)
    mode = batch.mode_results()
    arr = batch.array_results()
    l64 = batch._host("llks64", (U, G))
    plain = ExactDeviceBatch(reads, K, haps, counts, prior, cache_joint=False)
    assert plain.ws_bytes < batch.ws_bytes, "the cached second pass was not taken"
    plain.run(streaming=True, arrays=False)
    for a, b in zip(mode, plain.mode_results()):
        assert np.array_equal(a, b, equal_nan=True), "cached and plain second passes differ"
    for u in range(U):
        ru, cu = oracle_inputs[u] if oracle_inputs is not None else (reads[u], None if counts is None else counts[u])
        pr = None if prior is None else (float(prior[0][u]), None if prior[1] is None else prior[1][u])
        e32, e64 = orc.genotype_likelihoods(ru, K, haps[u], cu)
        a, ml, mp, sp, fq, oc = orc.posterior_mode(ru, K, haps[u], cu, pr)
        # ---- streaming form ----
        got = mode[0][u]
        if got.tolist() == a.tolist():
            np.testing.assert_allclose([mode[1][u], mode[2][u], mode[3][u]], [ml, mp, sp], rtol=1e-9, err_msg="unit %d" % u)
        else:
            assert not exact_ties, ("unit %d: mode %s, oracle %s (exact tie: the first genotype wins)" % (u, got.tolist(), a.tolist()))
            i_dev, i_orc = calling.genotype_alleles_as_index(got), calling.genotype_alleles_as_index(a)
            lj = e64 + _log_prior(G, K, H, pr)
            assert abs(lj[i_dev] - lj[i_orc]) <= 1e-12 * max(abs(lj[i_orc]), 1.0), (
                "unit %d: mode %s (joint %r), oracle %s (joint %r)" % (u, got.tolist(), lj[i_dev], a.tolist(), lj[i_orc]))
            p64 = orc.genotype_posteriors(e64, K, H, pr)
            sp_dev = calling.alternate_dosage_posteriors(got, p64)[1].sum()
            np.testing.assert_allclose([mode[1][u], mode[2][u], mode[3][u]], [e64[i_dev], p64[i_dev], sp_dev], rtol=1e-9)
        np.testing.assert_allclose(mode[4][u], fq, rtol=1e-9, atol=1e-300, err_msg="freqs, unit %d" % u)
        np.testing.assert_allclose(mode[5][u], oc, rtol=1e-9, atol=1e-300, err_msg="occur, unit %d" % u)
        # ---- array form ----
        np.testing.assert_allclose(arr["llks"][u], e32, rtol=2.5e-7, err_msg="float32 llks, unit %d" % u)
        np.testing.assert_allclose(l64[u], e64, rtol=1e-10, err_msg="float64 llks, unit %d" % u)
        ref = orc.genotype_posteriors(e32, K, H, pr)
        ptol = max(3e-5, 4 * float(np.spacing(np.float32(np.abs(e32).max()))))
        post = arr["posteriors"][u]
        np.testing.assert_allclose(post, ref, rtol=ptol, atol=1e-12, err_msg="posteriors, unit %d" % u)
        idx = int(np.argmax(post))
        assert arr["alleles"][u].tolist() == calling.index_as_genotype_alleles(idx, K).tolist(), "array mode, unit %d" % u
        assert arr["prob"][u] == post[idx]
        rf, rc_, ro = orc.posterior_allele_frequencies(post, K, H)
        np.testing.assert_allclose(np.stack([arr["freqs"][u], arr["counts"][u], arr["occur"][u]]), np.stack([rf, rc_, ro]),
                                   rtol=1e-9, atol=1e-300, err_msg="array frequencies, unit %d" % u)
        ap = calling.alternate_dosage_posteriors(arr["alleles"][u], post)[1]
        np.testing.assert_allclose(arr["support_prob"][u], ap.sum(), rtol=1e-12)
        # ---- the two forms name the same mode (the array form's posteriors come from float32 likelihoods: where they put the
        # streaming mode within their own tolerance of the maximum, either genotype is the array form's to take)
        if arr["alleles"][u].tolist() != got.tolist():
            assert not exact_ties, "unit %d: array mode %s, streaming mode %s" % (u, arr["alleles"][u].tolist(), got.tolist())
            i_dev = calling.genotype_alleles_as_index(got)
            assert post[i_dev] >= post[idx] * (1 - ptol), "unit %d: array mode %s, streaming mode %s" % (u, arr["alleles"][u].tolist(), got.tolist())
    return batch


def draw_case(rng):
    """One random shape within the oracle's time (G * R * K <= about 2e8 and G <= 10^6 per unit)."""
    K = int(rng.integers(1, 16))
    M = int(rng.integers(1, 13))
    A = int(rng.integers(2, 5))
    na = rng.integers(2, A + 1, size=M)
    na[rng.integers(0, M)] = A
    n_haps = int(np.prod(na.astype(float)))
    H = int(rng.integers(2, 41))
    H = int(min(H, n_haps))
    R = int(rng.choice([1, 2, 3, 5, 17, 64, 203, 700, 1501, 2600]))
    while H > 2 and (comb(H + K - 1, K) * R * K > 2e8 or comb(H + K - 1, K) > 10 ** 6):
        H -= 1
    while R > 1 and comb(H + K - 1, K) * R * K > 2e8:
        R = max(1, R // 2)
    return K, H, na, R


def run(n_cases, seed, only=None, verbose=False):
    from tests.helpers import multiallelic_units

    rng = np.random.default_rng(seed)
    bad = 0
    for case in range(n_cases):
        K, H, na, R = draw_case(rng)
        U = int(rng.integers(1, 4))
        s_ = int(rng.integers(0, 2 ** 31))
        ckind = int(rng.integers(0, 4))
        pkind = int(rng.integers(0, 3))
        if only is not None and case != only:
            continue
        r2 = np.random.default_rng(s_)
        reads, haps = multiallelic_units(r2, U, K, H, na, R, qual=(2, 30), gap=float(r2.choice([0.0, 0.1, 0.4])))
        counts = [None, np.ones((U, R), np.int64), r2.integers(1, 5, size=(U, R)), r2.integers(0, 3, size=(U, R))][ckind]
        F = r2.choice([0.0, 0.05, 0.3], size=U)
        prior = [None, (F, None), (F, r2.dirichlet(np.ones(H), size=U))][pkind]
        path = exact_path(R, H, K, counts)
        desc = "case %d: K %d H %d n_alleles %s R %d U %d counts %s prior %s (G %d tiled %s blocks %d w01 %s)" % (
            case, K, H, na.tolist(), R, U, ["none", "ones", "1-4", "zeros"][ckind], ["none", "F", "F+freqs"][pkind],
            path["G"], path["tiled"], path["nblk"], path["w01"])
        if verbose:
            print(desc, flush=True)
        try:
            check_exact_batch(reads, K, haps, counts, prior)
        except AssertionError as e:
            bad += 1
            print("DIFFERENCE " + desc + "\n  " + str(e).strip().replace("\n", "\n  "), flush=True)
    print("fuzz_exact: %d cases, seed %d: %d differences" % (n_cases, seed, bad), flush=True)
    return bad


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    only = int(sys.argv[3]) if len(sys.argv) > 3 else None
    sys.exit(1 if run(n, sd, only, verbose=True) else 0)
