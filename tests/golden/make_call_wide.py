#!/usr/bin/env python3
"""Generate tests/golden/call_wide.npz: `mchap call` over 300 known haplotypes at ploidy 2 (45 150 genotypes), the input and the
reference's own answers -- the posterior allele frequencies of its exact caller over all genotypes, and those of its sampler
(CallingMCMC, Gibbs and Metropolis-Hastings, 25 000 steps x 2 chains, burn 1000) run under the identity-njit stand-ins of tests/golden/_shim (numpy's legacy
MT19937 generator; see make_golden.py).  The sampler's distance from the exact frequencies is the yardstick of the 0.015 tolerance of
tests/test_gpu_call_wide.py: the fixture records it per step type (`ref_max_abs_diff`, `ref_mh_max_abs_diff`, `steps`).

Runs ONLY where the reference is at hand.  Output: data only (inputs and recorded results).
Usage:  python tests/golden/make_call_wide.py [steps]
"""
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")
sys.path.append(ROOT)

import numpy as np  # noqa: E402

warnings.simplefilter("ignore")

from mchap.calling import exact as ref_exact  # noqa: E402
from mchap.calling.classes import CallingMCMC  # noqa: E402

K, H, M, R, BURN, CHAINS, SEED = 2, 300, 10, 14, 1000, 2, 11


def make_input():
    """14 low-quality reads of a diploid over 10 biallelic SNVs; 300 distinct known haplotypes, the true ones among them."""
    from mchap_amd.synth import synth_units

    rng = np.random.default_rng(300)
    reads, _, truth = synth_units(1, ploidy=K, n_pos=M, n_reads=R, first_unit=31, window=(2, M), qual=(3, 10))
    pool = np.unique(np.concatenate([truth[0], rng.integers(0, 2, size=(6 * H, M)).astype(np.int8)]), axis=0)
    rng.shuffle(pool)
    keep = [i for i, h in enumerate(pool) if any((h == t).all() for t in truth[0])]
    rest = [i for i in range(len(pool)) if i not in keep]
    idx = np.array(keep + rest[: H - len(keep)])
    rng.shuffle(idx)
    haps = pool[idx]
    assert haps.shape == (H, M) and len(np.unique(haps, axis=0)) == H
    return np.ascontiguousarray(reads[0]), haps.astype(np.int8)


def _fit(args):
    step_type, steps = args
    reads, haps = make_input()
    t0 = time.time()
    trace = CallingMCMC(ploidy=K, haplotypes=haps, prior=None, steps=steps, chains=CHAINS, random_seed=SEED, step_type=step_type).fit(reads)
    g = np.asarray(trace.genotypes)[:, BURN:].reshape(-1)
    return np.bincount(g, minlength=H) / float(len(g)), time.time() - t0


def main():
    from multiprocessing import Pool

    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 25000
    reads, haps = make_input()
    llks = ref_exact.genotype_likelihoods(reads, K, haps)
    post = ref_exact.genotype_posteriors(llks, K, H, None)
    exact_freqs, _, _ = ref_exact.posterior_allele_frequencies(post, K, H)
    with Pool(2) as pool:  # (each step type in a process of its own: each seeds numpy's generator itself)
        (gibbs, tg), (mh, tm) = pool.map(_fit, [("Gibbs", steps), ("Metropolis-Hastings", steps)])
    diff = float(np.abs(gibbs - exact_freqs).max())
    diff_mh = float(np.abs(mh - exact_freqs).max())
    print("steps %d: reference sampler vs exact: max |d freq| = %.5f Gibbs (%.0f s), %.5f Metropolis-Hastings (%.0f s)" % (steps, diff, tg, diff_mh, tm))
    np.savez_compressed(os.path.join(HERE, "call_wide.npz"), reads=reads, haplotypes=haps, ploidy=np.array(K), steps=np.array(steps),
                        chains=np.array(CHAINS), burn=np.array(BURN), ref_exact_freqs=np.asarray(exact_freqs, dtype=np.float64),
                        ref_mcmc_freqs=gibbs, ref_max_abs_diff=np.array(diff), ref_mh_freqs=mh, ref_mh_max_abs_diff=np.array(diff_mh))


if __name__ == "__main__":
    main()
