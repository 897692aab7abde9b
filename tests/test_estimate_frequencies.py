"""call-exact --estimate-prior-frequencies on the host: the definition (application.estimate_frequencies_host on the oracle) against
an independent brute force and against the reference's own loop (tests/golden/estimate_frequencies.npz), the stopping rule, the
command line and the resident / recompute plan.  CPU only."""
import io as _io
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from mchap_amd import application
from tests.estimate_units import brute_iterate, close, fresh, make_record, per_sample, samples_of

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# 1e-10 relative for llk and prior arithmetic in float64; applied to the frequencies with an absolute floor of 1e-12
REL, FLOOR = 1e-10, 1e-12

# name: (H, M, ploidies, reads per sample, inbreeding per sample, REFMASKED)
SHAPES = {
    "H3_K2": (3, 2, (2, 2, 2), (10, 7, 12), (0.1, 0.1, 0.1), False),
    "H4_K4": (4, 3, (4, 4), (16, 11), (0.2, 0.05), False),
    "ploidies_2_and_4": (4, 2, (2, 4, 2), (9, 15, 8), (0.1, 0.3, 0.0), False),
    "refmasked": (4, 3, (2, 2), (10, 12), (0.1, 0.1), True),
    "sample_without_reads": (3, 2, (2, 2, 4), (10, 0, 9), (0.1, 0.2, 0.1), False),
}


@pytest.fixture(scope="module")
def oracle():
    from tests.replay_call_exact import OracleBackend

    return OracleBackend()


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_definition_against_brute_force(name, oracle):
    H, M, ploidies, n_reads, inbreeding, masked = SHAPES[name]
    unit = make_record(np.random.default_rng(11 + len(name)), H, M, ploidies, n_reads, masked=masked)
    want = brute_iterate(unit, ploidies, inbreeding, 5)
    for n in (1, 5):
        units = fresh([unit])
        out = application.estimate_prior_frequencies(units, samples_of(units), per_sample(ploidies), per_sample(inbreeding), n,
                                                     tolerance=0.0, backend=oracle)
        f, it = out[0]
        ok, dev = close(f, want[n - 1], REL, FLOOR)
        print(name, n, "max deviation", dev)
        assert it == n and units[0]["emit"] == n and ok, (f, want[n - 1])
        assert np.array_equal(units[0]["locus"].frequencies, f)
        assert abs(f.sum() - 1.0) < 1e-12
        if masked:
            assert f[0] == 0.0


def test_the_definition_against_the_reference_loop(oracle):
    z = np.load(os.path.join(GOLDEN, "estimate_frequencies.npz"))
    assert int(z["n_records"]) == 2 and int(z["rounds"]) == 5
    for i in range(int(z["n_records"])):
        ploidies, inbreeding = [int(k) for k in z["ploidy_%d" % i]], [float(x) for x in z["inbreeding_%d" % i]]
        haps = z["haps_%d" % i]
        reads = {"S%d" % s: dict(dists=z["dists_%d_%d" % (i, s)], counts=z["counts_%d_%d" % (i, s)]) for s in range(len(ploidies))}
        for n in range(1, 6):
            locus = SimpleNamespace(haplotypes=haps, frequencies=np.array(z["f0_%d" % i]), n_alleles=[2] * haps.shape[1])
            units = [dict(rec={}, locus=locus, invalid=None, reads=reads, needs_kernel=True)]
            f, it = application.estimate_prior_frequencies(units, list(reads), per_sample(ploidies), per_sample(inbreeding), n,
                                                           tolerance=0.0, backend=oracle)[0]
            ok, dev = close(f, z["f_%d" % i][n - 1], REL, FLOOR)
            print("record", i, "round", n, "max deviation", dev)
            assert it == n and ok, (f, z["f_%d" % i][n - 1])
        if bool(z["masked_%d" % i]):
            assert f[0] == 0.0


class _Contraction:
    """A backend whose posterior frequencies move a fixed share of the way to a target: a record of 3 haplotypes closes 99 % of
    the gap per round, one of 4 haplotypes 10 %."""

    @staticmethod
    def posterior_mode(dists, ploidy, haps, read_counts=None, prior=None, **kw):
        H = len(haps)
        target = np.arange(1, H + 1) / (H * (H + 1) / 2)
        rate = 0.01 if H == 3 else 0.9
        return np.zeros(ploidy, int), 0.0, 1.0, 1.0, target + (np.asarray(prior[1]) - target) * rate, np.ones(H)


def _two_records():
    rng = np.random.default_rng(5)
    return [make_record(rng, 3, 2, (2, 2), (4, 4)), make_record(rng, 4, 2, (2, 2), (4, 4))]


def test_stopping_rule_and_iteration_counts():
    ploidy, inb = (lambda s: 2), (lambda s: 0.1)
    base = _two_records()
    run = lambda n, eps: application.estimate_prior_frequencies(fresh(base), samples_of(base), ploidy, inb, n, tolerance=eps, backend=_Contraction)
    # N = 0 leaves f_0
    units = fresh(base)
    out = application.estimate_prior_frequencies(units, samples_of(base), ploidy, inb, 0, tolerance=1e-2, backend=_Contraction)
    assert [units[i]["emit"] for i in (0, 1)] == [0, 0]
    assert all(np.array_equal(out[i][0], base[i]["locus"].frequencies) for i in (0, 1))
    # the first record's second round moves it by less than 1e-2 (0.99 x 0.01 of the first gap): it stops there, and the round
    # counts; its neighbour goes on to N
    # (the neighbour's fourth round still moves it by 0.1 x 0.9^3 x 0.15 = 0.0109)
    out = run(4, 1e-2)
    assert out[0][1] == 2 and out[1][1] == 4
    assert np.array_equal(out[0][0], run(2, 0.0)[0][0])      # the row of the round that met the tolerance, unchanged afterwards
    assert np.array_equal(out[1][0], run(4, 0.0)[1][0])
    assert not np.array_equal(out[0][0], run(1, 0.0)[0][0])
    # without a tolerance every record runs N rounds
    assert [v[1] for v in run(5, 0.0).values()] == [5, 5]
    # records that are not called are not estimated
    units = fresh(base)
    units[1]["needs_kernel"], units[1]["invalid"] = False, "AF0"
    out = application.estimate_prior_frequencies(units, samples_of(base), ploidy, inb, 3, backend=_Contraction)
    assert list(out) == [0] and units[1]["emit"] is None and units[0]["emit"] is not None


def test_estimate_needs_inbreeding_for_every_sample():
    base = _two_records()
    with pytest.raises(ValueError, match="inbreeding"):
        application.estimate_prior_frequencies(fresh(base), samples_of(base), lambda s: 2, lambda s: None, 3, backend=_Contraction)
    with pytest.raises(ValueError, match="inbreeding"):
        application.estimate_prior_frequencies(fresh(base), samples_of(base), lambda s: 2, {"S0": 0.1, "S1": None}.get, 3, backend=_Contraction)
    with pytest.raises(ValueError, match="estimate_path"):
        application.estimate_prior_frequencies(fresh(base), samples_of(base), lambda s: 2, lambda s: 0.1, 3, backend=_Contraction, path="fast")


# ---- the program ----
def _cli(monkeypatch, oracle, extra):
    """`call-exact` of the golden job with prior frequencies through cli.run, the exact caller replaced by the oracle."""
    from mchap_amd import cli

    real = application.call_exact
    monkeypatch.setattr(application, "call_exact", lambda *a, **kw: real(*a, calling=oracle, **kw))
    argv = ["mchap_amd", "call-exact", "--haplotypes", os.path.join(HERE, "mock.input.frequencies.vcf"), "--ploidy", "4", "--bam"] + \
        [os.path.join(HERE, f) for f in ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")] + \
        ["--report", "AFPRIOR", "AFP"] + extra
    out = _io.StringIO()
    cli.run(argv, out)
    lines = out.getvalue().splitlines()
    return [ln for ln in lines if ln.startswith("#")], [ln for ln in lines if not ln.startswith("#")]


def _decl(lines):
    return [ln for ln in lines if ln.startswith(("##FILTER", "##INFO", "##FORMAT", "##contig", "#CHROM")) and not ln.startswith("##FILTER=<ID=LIMIT,")]


def test_command_line(monkeypatch, oracle):
    golden = [ln.rstrip("\n") for ln in open(os.path.join(HERE, "simple.output.mixed_depth.call-exact.frequencies.prior.vcf"))]
    prior = ["--use-dirmul-prior", "0.0", "AFP"]
    # without the flags: header and records of the golden job, unchanged
    head, recs = _cli(monkeypatch, oracle, prior)
    assert _decl(head) == _decl([ln for ln in golden if ln.startswith("#")])
    assert recs == [ln for ln in golden if not ln.startswith("#")]
    assert not any("EMIT" in ln for ln in head + recs)
    # with them: one more declaration, after the other INFO fields, and EMIT at the end of every record's INFO
    monkeypatch.undo()
    head2, recs2 = _cli(monkeypatch, oracle, prior + ["--estimate-prior-frequencies", "3", "--estimate-tolerance", "0"])
    decl = '##INFO=<ID=EMIT,Number=1,Type=Integer,Description="Iterations of the prior allele-frequency estimate run for the record">'
    assert decl in head2 and [ln for ln in _decl(head2) if ln != decl] == _decl(head)
    info = [ln for ln in head2 if ln.startswith("##INFO")]
    assert info[-1] == decl
    assert len(recs2) == len(recs)
    n_estimated = 0
    for a, b in zip(recs, recs2):
        ca, cb = a.split("\t"), b.split("\t")
        emit = cb[7].rsplit(";", 1)[1]
        assert emit in ("EMIT=3", "EMIT=.") and ca[:7] == cb[:7]
        n_estimated += emit == "EMIT=3"
        if emit == "EMIT=.":   # nothing estimated: the record as it is written today
            assert cb[7].rsplit(";", 1)[0] == ca[7] and ca[8:] == cb[8:]
    assert n_estimated >= 1
    # N = 0: every record as today, with EMIT = 0 where it would have been estimated
    monkeypatch.undo()
    _, recs0 = _cli(monkeypatch, oracle, prior + ["--estimate-prior-frequencies", "0"])
    assert [re.sub(r";EMIT=[^\t;]*", "", ln) for ln in recs0] == recs and any(";EMIT=0\t" in ln for ln in recs0)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="--estimate-tolerance needs"):
        _cli(monkeypatch, oracle, prior + ["--estimate-tolerance", "1e-4"])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="--use-dirmul-prior"):
        _cli(monkeypatch, oracle, ["--estimate-prior-frequencies", "3"])
    from mchap_amd import cli

    text = cli.build_parser("call-exact").format_help()
    for flag in ("--estimate-prior-frequencies", "--estimate-tolerance"):
        assert " ".join(text.rsplit(flag, 1)[1].split())[:40].endswith("(not a reference flag)") or \
            "(not a reference flag)" in " ".join(text.rsplit(flag, 1)[1].split())[:40]
        assert flag not in cli.build_parser("call").format_help()


def test_keyword_off_is_todays_output_and_the_estimate_is_the_prior_used(oracle):
    vcf = os.path.join(HERE, "mock.input.frequencies.vcf")
    bams = {s: os.path.join(HERE, f) for s, f in zip(["SAMPLE1", "SAMPLE2", "SAMPLE3"],
                                                     ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam"))}
    kw = dict(report=("AFPRIOR", "AFP"), prior_frequencies_tag="AFP", inbreeding=0.1, calling=oracle)
    plain = list(application.call_exact(vcf, bams, **kw))
    assert list(application.call_exact(vcf, bams, estimate_frequencies=None, **kw)) == plain
    once = list(application.call_exact(vcf, bams, estimate_frequencies=1, estimate_tolerance=0.0, **kw))
    # one round from the tag's values: the prior the call used (AFPRIOR) is the AFP a plain run reports, at the VCF's decimals
    n = 0
    for a, b in zip(plain, once):
        ia, ib = dict(x.split("=") for x in a.split("\t")[7].split(";") if "=" in x), dict(x.split("=") for x in b.split("\t")[7].split(";") if "=" in x)
        if ib["EMIT"] == "1":
            assert ib["AFPRIOR"] == ia["AFP"]
            n += 1
    assert n >= 1
    # sharding by records and the record blocks do not change a record
    assert list(application.call_exact(vcf, bams, estimate_frequencies=1, estimate_tolerance=0.0, records_per_block=1, **kw)) == once
    parts = [ln for r in range(2) for ln in application.call_exact(vcf, bams, estimate_frequencies=1, estimate_tolerance=0.0, shard=(r, 2), **kw)]
    assert parts == once


# ---- the plan ----
def test_a_record_over_the_budget_goes_to_recompute_and_its_neighbours_stay_resident(monkeypatch):
    from math import comb

    rng = np.random.default_rng(3)
    units = [make_record(rng, 3, 2, (2, 4), (2, 2)), make_record(rng, 16, 4, (2, 4), (2, 2)), make_record(rng, 4, 2, (2, 4), (2, 2)),
             make_record(rng, 3, 2, (2, 4), (2, 2))]
    units[3]["needs_kernel"] = False
    cost = lambda H: sum(application._exact_unit_bytes(comb(H + K - 1, K), 8) for K in (2, 4))
    assert cost(16) > cost(4) + cost(3)
    asked = []

    def budget(bytes_per_unit, **kw):
        asked.append(bytes_per_unit)
        return (cost(16) - 1) // bytes_per_unit

    monkeypatch.setattr(application, "device_unit_budget", budget)
    samples = samples_of(units)
    resident, recompute, refused = application._estimate_plan(units, samples, per_sample((2, 4)))
    assert resident == [[0, 2]] and recompute == [[1]] and refused == [] and asked == [1]
    # a budget that holds one small record at a time: sub-blocks of whole records
    monkeypatch.setattr(application, "device_unit_budget", lambda b, **kw: cost(4) // b)
    assert application._estimate_plan(units, samples, per_sample((2, 4))) == ([[0], [2]], [[1]], [])
    # the keyword forces either path; a shape the library refuses is not estimated
    assert application._estimate_plan(units, samples, per_sample((2, 4)), "recompute") == ([], [[0, 1, 2]], [])
    assert application._estimate_plan(units, samples, per_sample((2, 4)), "resident") == ([[0], [1], [2]], [], [])
    assert application._estimate_plan(units, samples, per_sample((2, 16))) == ([], [], [0, 1, 2])
    # the same cost of a unit as the exact caller's own chunks
    assert application._exact_unit_bytes(35, 8, 10, 3, 2, 4) == 10 * 3 * 2 * 8 + 10 * 8 + 4 * 3 + 35 * 8 + 4096
