"""call-exact --estimate-prior-frequencies on the device: the counts and update kernels over resident likelihoods
(mchap_exact_em_counts_device, mchap_exact_em_update_device) against the oracle-backed definition and against the recompute path,
whole runs, determinism, freezing, and the program on the reference's test files."""
import os

import numpy as np
import pytest

from mchap_amd import application
from tests.estimate_units import close, fresh, make_record, per_sample, samples_of

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
# 1e-9 relative for the fp64 exact posterior, applied to the frequencies with an absolute floor of 1e-12
REL, FLOOR = 1e-9, 1e-12

# name: (H, M, ploidies, reads per sample (at most 40), inbreeding per sample, REFMASKED)
SHAPES = {
    "G6": (3, 2, (2, 2, 2), (10, 7, 12), (0.1, 0.1, 0.1), False),
    "G35": (4, 3, (4, 4), (16, 11), (0.2, 0.05), False),
    "G12376_several_blocks": (12, 4, (6, 6), (40, 25), (0.1, 0.2), False),
    "K10_KM16": (3, 2, (10, 10), (30, 40), (0.1, 0.3), False),
    "ploidies_2_and_4": (4, 2, (2, 4, 2), (9, 15, 8), (0.1, 0.3, 0.0), False),
    "refmasked": (4, 3, (2, 2), (10, 12), (0.1, 0.1), True),
    "sample_without_reads": (3, 2, (2, 2, 4), (10, 0, 9), (0.1, 0.2, 0.1), False),
}


def _oracle():
    from tests.replay_call_exact import OracleBackend

    return OracleBackend()


def _run(units, ploidies, inbreeding, n, eps, **kw):
    u = fresh(units)
    out = application.estimate_prior_frequencies(u, samples_of(u), per_sample(ploidies), per_sample(inbreeding), n, tolerance=eps, **kw)
    assert [x["emit"] for x in u] == [out[i][1] for i in range(len(u))]
    return out


@pytest.fixture(scope="module")
def one_iteration():
    """Per shape: f_1 by the oracle-backed definition, by the resident path and by the recompute path (computed once)."""
    got = {}
    for name, (H, M, ploidies, n_reads, inbreeding, masked) in SHAPES.items():
        unit = make_record(np.random.default_rng(100 + len(name)), H, M, ploidies, n_reads, masked=masked)
        got[name] = {k: _run([unit], ploidies, inbreeding, 1, 0.0, **kw)[0]
                     for k, kw in (("oracle", dict(backend=_oracle())), ("resident", dict(path="resident")), ("recompute", dict(path="recompute")))}
    return got


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_iteration_of_the_kernels_against_the_definition(name, one_iteration):
    (f, it), (want, _) = one_iteration[name]["resident"], one_iteration[name]["oracle"]
    ok, dev = close(f, want, REL, FLOOR)
    print(name, "resident vs oracle: max deviation %.3g" % dev)
    assert it == 1 and ok, (f, want)
    if SHAPES[name][5]:
        assert f[0] == 0.0 and want[0] == 0.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_iteration_resident_against_recompute(name, one_iteration):
    (f, it), (want, it2) = one_iteration[name]["resident"], one_iteration[name]["recompute"]
    ok, dev = close(f, want, REL, FLOOR)
    print(name, "resident vs recompute: max deviation %.3g" % dev)
    assert it == 1 and it2 == 1 and ok, (f, want)
    ok, dev = close(want, one_iteration[name]["oracle"][0], REL, FLOOR)
    print(name, "recompute vs oracle: max deviation %.3g" % dev)
    assert ok


# three records of one block: 3, 4 and 5 haplotypes (rows of different lengths in one slab), samples of ploidy 2 and 4 (two shape
# groups feed every record)
PLOIDIES, INBREEDING = (2, 4, 2), (0.1, 0.3, 0.05)


@pytest.fixture(scope="module")
def three_records():
    rng = np.random.default_rng(77)
    return [make_record(rng, 3, 2, PLOIDIES, (12, 20, 0)), make_record(rng, 4, 3, PLOIDIES, (9, 14, 11), masked=True),
            make_record(rng, 5, 3, PLOIDIES, (25, 8, 16))]


def test_whole_run_against_the_definition(three_records):
    N = 20
    oracle = _oracle()
    want = _run(three_records, PLOIDIES, INBREEDING, N, 0.0, backend=oracle)
    # the amplification of these inputs: the definition from f_0 and from f_0 perturbed by 1e-9 relative
    rng = np.random.default_rng(1)
    moved = fresh(three_records)
    first = 0.0
    for u in moved:
        f = u["locus"].frequencies
        g = f * (1.0 + 1e-9 * rng.choice([-1.0, 1.0], size=len(f)))
        first = max(first, float(np.max(np.abs(g - f) / np.where(f > 0, f, 1.0))))
        u["locus"].frequencies = g
    other = _run(moved, PLOIDIES, INBREEDING, N, 0.0, backend=oracle)
    spread = max(float(np.max(np.abs(other[i][0] - want[i][0]) / np.where(want[i][0] > FLOOR, want[i][0], 1.0))) for i in range(3))
    A = spread / first
    bound = 10 * 1e-9 * max(1.0, A)
    got = _run(three_records, PLOIDIES, INBREEDING, N, 0.0, path="resident")
    worst = 0.0
    for i in range(3):
        ok, dev = close(got[i][0], want[i][0], bound, FLOOR)
        worst = max(worst, float(np.max(np.abs(got[i][0] - want[i][0]) / np.where(want[i][0] > FLOOR, want[i][0], 1.0))))
        assert got[i][1] == N and want[i][1] == N and ok, (i, got[i][0], want[i][0])
    print("whole run: amplification A = %.3g, bound %.3g relative, measured %.3g relative" % (A, bound, worst))
    assert got[1][0][0] == 0.0
    # the recompute path through the same run
    again = _run(three_records, PLOIDIES, INBREEDING, N, 0.0, path="recompute")
    for i in range(3):
        assert close(again[i][0], want[i][0], bound, FLOOR)[0] and again[i][1] == N


def test_equal_bits_on_every_run_and_however_often_the_host_looks(three_records):
    runs = [_run(three_records, PLOIDIES, INBREEDING, 20, 1e-6, path="resident", poll=p) for p in (4, 4, 1, 8)]
    for other in runs[1:]:
        for i in range(3):
            assert other[i][1] == runs[0][i][1]
            assert other[i][0].tobytes() == runs[0][i][0].tobytes()


def test_a_frozen_record_keeps_the_row_of_the_iteration_it_stopped_at(three_records):
    N = 8
    rows = [_run(three_records, PLOIDIES, INBREEDING, t, 0.0, path="resident") for t in range(1, N + 1)]
    f0 = [u["locus"].frequencies for u in three_records]
    delta = [[float(np.max(np.abs(rows[t][i][0] - (rows[t - 1][i][0] if t else f0[i])))) for t in range(N)] for i in range(3)]
    # a tolerance between two records' third steps: one of them stops at iteration 3 at the latest, the other goes on
    third = sorted(d[2] for d in delta)
    assert third[0] < third[-1]
    eps = 0.5 * (third[0] + third[1])
    stop = [next((t + 1 for t in range(N) if delta[i][t] < eps), N) for i in range(3)]
    print("deltas", delta, "eps", eps, "stop", stop)
    assert min(stop) < N and len(set(stop)) > 1
    got = _run(three_records, PLOIDIES, INBREEDING, N, eps, path="resident", poll=1)
    for i in range(3):
        assert got[i][1] == stop[i]
        assert got[i][0].tobytes() == rows[stop[i] - 1][i][0].tobytes()


def test_n_zero_and_the_plan_on_the_device(three_records, monkeypatch):
    got = _run(three_records, PLOIDIES, INBREEDING, 0, 1e-6)
    for i in range(3):
        assert got[i][1] == 0 and np.array_equal(got[i][0], three_records[i]["locus"].frequencies)
    # a budget that sends the record of 5 haplotypes to the recompute path and keeps the others resident: the same estimate
    from math import comb

    cost = lambda H: sum(application._exact_unit_bytes(comb(H + K - 1, K), 8) for K in PLOIDIES)
    want = _run(three_records, PLOIDIES, INBREEDING, 3, 0.0, path="resident")
    real = application.device_unit_budget
    monkeypatch.setattr(application, "device_unit_budget", lambda b, **kw: (cost(5) - 1) // b if b == 1 else real(b, **kw))
    assert application._estimate_plan(three_records, samples_of(three_records), per_sample(PLOIDIES))[:2] == ([[0], [1]], [[2]])
    got = _run(three_records, PLOIDIES, INBREEDING, 3, 0.0)
    for i in range(3):
        assert close(got[i][0], want[i][0], REL, FLOOR)[0] and got[i][1] == 3


@pytest.mark.parametrize("block_path", [False, True])
def test_the_program_calls_with_the_estimate(block_path, tmp_path):
    from mchap_amd.io import vcfstr

    vcf = os.path.join(HERE, "simple.output.mixed_depth.assemble.vcf")
    paths = {s: os.path.join(HERE, f) for s, f in zip(["SAMPLE1", "SAMPLE2", "SAMPLE3"],
                                                      ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam"))}
    source = application.ReadSource(paths)
    kw = dict(ploidy=4, inbreeding=0.1, report=("AFPRIOR", "AFP"), block_path=block_path)
    lines = list(application.call_exact(vcf, source, estimate_frequencies=5, **kw))
    # the estimate itself, unrounded
    _, records = application.read_vcf(vcf)
    samples = source.samples
    units = application._exact_units(records, source, samples, None, None, block_path)
    est = application.estimate_prior_frequencies(units, samples, lambda s: 4, lambda s: 0.1, 5)
    assert len(est) >= 1 and len(lines) == len(records)
    # a copy of the VCF whose INFO carries the estimate written with repr, called as today with --prior-frequencies on that tag
    copy, ri = [], 0
    for ln in open(vcf):
        if ln.startswith("#CHROM"):
            copy.append('##INFO=<ID=EMF,Number=R,Type=Float,Description="estimated prior allele frequencies">\n')
        if not ln.startswith("#"):
            cols = ln.rstrip("\n").split("\t")
            n = 1 + (0 if cols[4] == "." else len(cols[4].split(",")))
            f = est[ri][0] if ri in est else np.full(n, 1.0 / n)
            if ri in est and units[ri]["locus"].mask_reference_allele:
                f = np.where(np.arange(n) == 0, 1.0, f)   # (a masked reference allele's value is not read)
            tag = "EMF=" + ",".join(repr(float(x)) for x in f)
            cols[7] = tag if cols[7] in (".", "") else cols[7] + ";" + tag
            ln = "\t".join(cols) + "\n"
            ri += 1
        copy.append(ln)
    path = tmp_path / "estimated.vcf"
    path.write_text("".join(copy))
    plain = list(application.call_exact(str(path), source, prior_frequencies_tag="EMF", **kw))
    assert len(plain) == len(lines)
    for i, (a, b) in enumerate(zip(lines, plain)):
        cols = a.split("\t")
        info = cols[7].split(";")
        assert info[-1] == ("EMIT=%d" % est[i][1] if i in est else "EMIT=.")
        assert "\t".join(cols[:7] + [";".join(info[:-1])] + cols[8:]) == b
        if i in est:
            afprior = [x for x in info if x.startswith("AFPRIOR=")][0]
            assert afprior == "AFPRIOR=" + vcfstr(np.asarray(est[i][0]))
