#!/usr/bin/env python3
"""Generate tests/golden/call_wide.npz: `mchap call` over 300 known haplotypes at ploidy 2 (45 150 genotypes), the input and the
reference's own answers -- the posterior allele frequencies of its exact caller over all genotypes, and those of its sampler
(CallingMCMC, Gibbs and Metropolis-Hastings, 25 000 steps x 2 chains, burn 1000) run under the identity-njit stand-ins of tests/golden/_shim (numpy's legacy
MT19937 generator; see make_golden.py).  The sampler's distance from the exact frequencies is the yardstick of the 0.015 tolerance of
tests/test_gpu_call_wide.py: the fixture records it per step type (`ref_max_abs_diff`, `ref_mh_max_abs_diff`, `steps`).

With `traces` it writes tests/golden/call_wide_traces.npz instead: the reference's sampler over MORE THAN 256 known haplotypes,
a few steps of it -- seeded CallingMCMC.fit traces of both step types, a seeded fit from a given initial genotype, the greedy
initial genotype and the transition vectors of gibbs_options / mh_options at states with alleles above 255 -- which pin the
oracle where its option arrays used to end (tests/test_call_wide.py).

Runs ONLY where the reference is at hand.  Output: data only (inputs and recorded results).
Usage:  python tests/golden/make_call_wide.py [steps]
        python tests/golden/make_call_wide.py traces
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


# (K, H, M, prior kind, read counts): the inputs are tests/call_wide_helpers.many_haplotypes(1, K, H, M, 12, seed=H + K, qual=(2, 8)) --
# twelve poor reads, so that the chains move
TRACE_CASES = [(4, 300, 10, None, False), (3, 321, 10, "Ff", True), (2, 1024, 10, None, True), (2, 300, 9, "F", False)]
# (Metropolis-Hastings proposes one of H - 1 alleles uniformly and accepts few: a longer run, so that its traces move too)
TRACE_STEPS, TRACE_CHAINS, TRACE_INI_STEPS, TRACE_MH_STEPS = 6, 2, 4, 40


def make_traces():
    """call_wide_traces.npz, case by case in the layout of call_mcmc.npz (make_golden.py gen_call_mcmc)."""
    from mchap.calling import mcmc as ref_cm
    from tests.call_wide_helpers import many_haplotypes

    out = {}
    for n, (Kc, Hc, Mc, kind, with_counts) in enumerate(TRACE_CASES):
        t0 = time.time()
        rng = np.random.default_rng(1000 * Kc + Hc)
        reads, haps = many_haplotypes(1, Kc, Hc, Mc, 12, seed=Hc + Kc, qual=(2, 8))
        reads, haps = np.ascontiguousarray(reads[0]), np.ascontiguousarray(haps[0])
        counts = rng.integers(1, 4, size=len(reads)).astype(np.int64) if with_counts else None
        fr = rng.dirichlet(np.ones(Hc))
        prior = {None: None, "F": (0.2, None), "Ff": (0.1, fr)}[kind]
        pre = "c%d_" % n
        out[pre + "haps"] = haps
        out[pre + "reads"] = reads
        out[pre + "counts"] = np.zeros(0, np.int64) if counts is None else counts
        out[pre + "meta"] = np.array([Kc, -1.0 if prior is None else prior[0], 0 if (prior is None or prior[1] is None) else 1])
        out[pre + "freqs"] = fr
        states, vecs = [], []
        for t in range(3):  # states whose alleles reach beyond 255: the top allele itself, then random ones
            g = rng.integers(0, Hc, size=Kc).astype(np.int64)
            g[t % Kc] = Hc - 1 if t == 0 else int(rng.integers(256, Hc))
            k = int(rng.integers(0, Kc))
            row = []
            for fn in (ref_cm.gibbs_options, ref_cm.mh_options):
                llks, lpri, probs = np.zeros(Hc), np.zeros(Hc), np.zeros(Hc)
                fn(g.copy(), k, haps, reads, counts, llks, lpri, probs, prior, None)
                row.append(np.stack([llks, lpri, probs]))
            states.append(np.append(g, k))
            vecs.append(np.stack(row))
        out[pre + "states"] = np.array(states)
        out[pre + "vectors"] = np.array(vecs)  # [3][2 (gibbs, mh)][3 (llk, lprior, prob)][H]
        out[pre + "greedy"] = ref_cm.greedy_caller(haps, Kc, reads, counts, prior).astype(np.int64)
        for st, name in ((0, "Gibbs"), (1, "Metropolis-Hastings")):
            model = CallingMCMC(ploidy=Kc, haplotypes=haps, prior=prior, steps=TRACE_MH_STEPS if st else TRACE_STEPS, chains=TRACE_CHAINS, random_seed=100 + n, step_type=name)
            tr = model.fit(reads, read_counts=counts)
            out[pre + "trace%d_g" % st] = np.asarray(tr.genotypes).astype(np.int64)
            out[pre + "trace%d_l" % st] = np.asarray(tr.llks)
        ini = np.sort(np.append(rng.integers(0, Hc, size=Kc - 1), Hc - 1)).astype(np.int64)
        model = CallingMCMC(ploidy=Kc, haplotypes=haps, prior=prior, steps=TRACE_INI_STEPS, chains=1, random_seed=7 + n)
        tr = model.fit(reads, read_counts=counts, initial=ini)
        out[pre + "initial"] = ini
        out[pre + "trace_ini_g"] = np.asarray(tr.genotypes).astype(np.int64)
        out[pre + "trace_ini_l"] = np.asarray(tr.llks)
        print("case %d (K %d, H %d, prior %s, counts %s): %.0f s" % (n, Kc, Hc, kind, with_counts, time.time() - t0), flush=True)
    out["n_cases"] = np.array(len(TRACE_CASES))
    out["steps"] = np.array([TRACE_STEPS, TRACE_CHAINS, TRACE_INI_STEPS, TRACE_MH_STEPS])
    np.savez_compressed(os.path.join(HERE, "call_wide_traces.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "traces":
        make_traces()
    else:
        main()
