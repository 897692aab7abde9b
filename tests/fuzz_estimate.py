"""Differential soak of the frequency-estimate kernels (exact_em_counts_kernel<8|16>, exact_em_combine_kernel,
exact_em_update_kernel through device.ExactFrequencyEstimate) against the long-double reference of one iteration
(tests/estimate_reference.py) on random shapes: 1-3 records of 2 <= G <= 20 000 genotypes, 1-6 samples of mixed ploidy 1-15,
F per sample from 0 / 1e-4 / 0.1 / 0.5 / 0.99, synthetic likelihood tables (uniform of three scales, peaked, with holes) and
frequency rows without zeros, with the reference allele masked, with the two highest alleles at 0 (tests/estimate_cases.py).
Also the driver tests/test_gpu_estimate_kernels.py runs its cases with.  Needs a GPU.  python tests/fuzz_estimate.py [cases] [seed]"""
import os
import sys
from math import comb

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# 1e-9 relative for the fp64 exact posterior, applied to the frequencies with an absolute floor of 1e-12
REL, FLOOR = 1e-9, 1e-12
MAX_G = 20000


def make_estimate(records, n_samples, ploidy_total, stride=None, rng=None):
    """A device.ExactFrequencyEstimate over `records` ([dict(H, f, units [(llk, K, F)], samples (the units' sample indices;
    default 0, 1, ...))]): one group per shape (H, K) with every record's units of that shape, in the order `rng` shuffles them
    into (None: as listed), rows of `stride` doubles (default: the largest H)."""
    import torch

    from mchap_amd.device import ExactFrequencyEstimate

    Hs = [int(r["H"]) for r in records]
    stride = max(Hs) if stride is None else int(stride)
    f0 = np.zeros((len(records), stride))
    for i, r in enumerate(records):
        f0[i, :Hs[i]] = r["f"]
    est = ExactFrequencyEstimate(np.array(Hs, dtype=np.int32), f0, n_samples, ploidy_total)
    groups = {}
    for i, r in enumerate(records):
        for s, (llk, K, F) in zip(r.get("samples", range(len(r["units"]))), r["units"]):
            assert llk.shape == (comb(Hs[i] + K - 1, K),) and llk.dtype == np.float64
            groups.setdefault((Hs[i], int(K)), []).append((i, int(s), llk, float(F)))
    for (H, K), members in groups.items():
        if rng is not None:
            members = [members[j] for j in rng.permutation(len(members))]
        llks = torch.from_numpy(np.concatenate([m[2] for m in members])).to(est.device)
        est.add_group(llks, H, K, [m[3] for m in members], [m[0] for m in members], [m[1] for m in members])
    return est


def reference_step(records, rows):
    """One iteration of the reference from `rows` (the records' current frequency rows; None: their f)."""
    from tests.estimate_reference import iterate

    return iterate([dict(r, f=r["f"] if rows is None else np.asarray(rows[i][:r["H"]])) for i, r in enumerate(records)])


def compare_step(records, before, after):
    """Every element of every record's new row against the reference applied to the row before: (all within REL / FLOOR, worst
    relative deviation).  Beyond that: a frequency that was 0 stays an exact 0, and so does the padding of the row."""
    from tests.estimate_reference import deviation

    ok, worst = True, 0.0
    for i, (r, want) in enumerate(zip(records, reference_step(records, before))):
        H = r["H"]
        got = after[i]
        o, dev = deviation(got[:H], want, REL, FLOOR)
        prev = np.asarray(r["f"] if before is None else before[i][:H])
        ok = ok and o and bool(np.all(got[:H][prev == 0.0] == 0.0)) and bool(np.all(got[H:] == 0.0))
        worst = max(worst, dev)
    return ok, worst


def draw_case(rng):
    """[records], ploidies of the samples: the ploidies first, then per record an H that keeps 2 <= G <= MAX_G for each of them
    (half of the records at the largest such H: that is where the tiles are)."""
    from tests import estimate_cases as cases

    n_samples = int(rng.integers(1, 7))
    pool = rng.integers(1, 16, size=2)
    ploidies = [int(pool[int(rng.integers(0, 2))]) for _ in range(n_samples)]
    Kmax = max(ploidies)
    Hmax = 2
    while Hmax < 200 and comb(Hmax + Kmax, Kmax) <= MAX_G:
        Hmax += 1
    Fs = cases.draw_inbreeding(rng, n_samples) if n_samples >= 2 else [float(rng.choice(cases.F_VALUES))]
    records = []
    for _ in range(int(rng.integers(1, 4))):
        H = Hmax if rng.random() < 0.5 else int(rng.integers(2, Hmax + 1))
        variant = str(rng.choice(cases.variants_for(H)))
        f = cases.frequency_row(rng, H, variant)
        kinds = [str(k) for k in rng.choice(cases.TABLE_KINDS, size=n_samples)]
        records.append(dict(H=H, f=f, variant=variant, kinds=kinds,
                            units=[(cases.likelihood_table(rng, H, ploidies[s], kinds[s], f), ploidies[s], Fs[s]) for s in range(n_samples)]))
    return records, ploidies


def drawn(n_cases, seed, only=None):
    """The cases of run(n_cases, seed), on the host alone: (case, records, ploidies, the paths its units take -- "KM8" / "KM16",
    "one tile" / "tiles" --, the case's generator)."""
    from tests.estimate_cases import TILE

    rng = np.random.default_rng(seed)
    for case in range(n_cases):
        s_ = int(rng.integers(0, 2 ** 31))
        if only is not None and case != only:
            continue
        r2 = np.random.default_rng(s_)
        records, ploidies = draw_case(r2)
        paths = set()
        for r in records:
            for _, K, _ in r["units"]:
                paths.add("KM8" if K <= 8 else "KM16")
                paths.add("one tile" if comb(r["H"] + K - 1, K) <= TILE else "tiles")
        yield case, records, ploidies, paths, r2


def run(n_cases, seed, only=None, verbose=False):
    """n_cases random cases, one step each against the reference; prints a line per case and returns the number that differ."""
    bad = 0
    for case, records, ploidies, paths, r2 in drawn(n_cases, seed, only):
        est = make_estimate(records, len(ploidies), sum(ploidies), rng=r2)
        est.step(0.0, 10 ** 6)
        rows, its = est.results()
        ok, worst = compare_step(records, None, rows)
        ok = ok and its.tolist() == [1] * len(records)
        desc = "case %d: ploidies %s H %s variants %s F %s (%s): worst %.3g relative" % (
            case, ploidies, [r["H"] for r in records], [r["variant"] for r in records], [u[2] for u in records[0]["units"]],
            ", ".join(sorted(paths)), worst)
        bad += not ok
        print(("" if ok else "DIFFERENCE ") + desc, flush=True)
    print("fuzz_estimate: %d cases, seed %d: %d differences" % (n_cases, seed, bad), flush=True)
    return bad


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    sd = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    only = int(sys.argv[3]) if len(sys.argv) > 3 else None
    sys.exit(1 if run(n, sd, only, verbose=True) else 0)
