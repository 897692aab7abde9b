"""call-exact --identity from the device: application.Identity over the simulated panel of tests/test_identity_host.py (its
conditions hold here too: seed 7, six records, two shape groups of samples -- tetraploids and diploids) against the host
definition on a float64 numpy likelihood backend: every LOG_BF within the bound of the kernel tests, summed over the records, and
the same row order; under a budget that forces the record-by-record path; and the program itself on the reference's alignment
files beside the other side files."""
import io as _io
import os
from math import comb

import numpy as np
import pytest

from tests import cross_reference
from tests import identity_reference as ref

pytestmark = pytest.mark.gpu

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")


@pytest.fixture(scope="module")
def block():
    from mchap_amd import application

    records, samples, matrices, ploidy_of = ref.panel()
    units = application._exact_units(records, application.MatrixSource(samples, matrices), samples, None, None, False)
    return units, samples, ploidy_of


def _compare(dev, host, units):
    """The same pairs in the same order, RECORDS and SKIPPED equal, every LOG_BF within the bound of a term times the records."""
    a, b = dev.table(), host.table()
    assert [(r["sample_1"], r["sample_2"], r["ploidy"], r["records"], r["skipped"]) for r in a] == \
        [(r["sample_1"], r["sample_2"], r["ploidy"], r["records"], r["skipped"]) for r in b]
    worst = 0.0
    for x, y in zip(a, b):
        floor = sum(ref.floor(comb(len(u["locus"].haplotypes) + x["ploidy"] - 1, x["ploidy"])) for u in units)
        err = abs(x["log_bf"] - y["log_bf"])
        worst = max(worst, err)
        assert err <= ref.REL * abs(y["log_bf"]) + floor, (x, y)
    print("largest |device - host| of a LOG_BF: %.3g" % worst)
    assert dev.text().split("\n")[:2] == host.text().split("\n")[:2]


@pytest.mark.parametrize("inbreeding", [None, 0.1], ids=["flat", "dirmul"])
def test_the_table_against_the_host_definition(block, inbreeding):
    from mchap_amd import application

    units, samples, ploidy_of = block
    dev = application.Identity(samples)
    got = dev.add_block(units, ploidy_of, lambda s: inbreeding)
    host = application.Identity(samples)
    want = host.add_block(units, ploidy_of, lambda s: inbreeding, cross_reference.NumpyBackend())
    assert set(got) == set(want) and all((got[k] is None) == (want[k] is None) for k in want)
    _compare(dev, host, units)
    first = dev.table()[0]
    assert (first["sample_1"], first["sample_2"], first["records"], first["skipped"]) == ref.DUPLICATE + (6, 0)
    assert first["log_bf"] > 20.0 and all(r["log_bf"] < -10.0 for r in dev.table()[1:])


def test_a_budget_forced_small_gives_the_same_table_record_by_record(block):
    from mchap_amd import application

    units, samples, ploidy_of = block
    flat = lambda s: None     # noqa: E731
    whole = application.Identity(samples)
    whole.add_block(units, ploidy_of, flat)
    need = max(application._identity_need(len(u["locus"].haplotypes), 4, 8) for u in units)
    cut = application.Identity(samples, budget=need)          # one record a launch
    cut.add_block(units, ploidy_of, flat)
    assert cut.sums == whole.sums and cut.skipped == whole.skipped and cut.records == whole.records
    assert cut.text() == whole.text()
    # a budget below the largest record's class skips that record for the class's pairs, and nothing else
    small = application.Identity(samples, budget=need - 1)
    small.add_block(units, ploidy_of, flat)
    big = sum(1 for u in units if application._identity_need(len(u["locus"].haplotypes), 4, 8) == need)
    assert 0 < big < len(units)
    for pair in small.plan.pairs:
        tetra = small.plan.key[pair[0]][0] == 4
        assert (small.records[pair], small.skipped[pair]) == ((len(units) - big, big) if tetra else (len(units), 0))
    host = application.Identity(samples, budget=need - 1)
    host.add_block(units, ploidy_of, flat, cross_reference.NumpyBackend())
    _compare(small, host, units)


def test_the_program_beside_the_other_side_files(tmp_path):
    from mchap_amd import cli

    bams = [os.path.join(HERE, f) for f in ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")]
    base = ["mchap_amd", "call-exact", "--haplotypes", os.path.join(HERE, "mock.input.frequencies.vcf"), "--ploidy", "4", "--bam"] + bams + \
        ["--use-dirmul-prior", "0.1", "AFP", "--estimate-prior-frequencies", "3"]
    cross = ["--cross-parents", "SAMPLE1", "SAMPLE2", "--parentage-candidates", "SAMPLE1", "SAMPLE2"]

    def run(extra):
        out = _io.StringIO()
        cli.run(base + extra, out)
        return out.getvalue()

    plain = run([])
    paths = {n: str(tmp_path / n) for n in ("i.tsv", "p.tsv", "cross.vcf", "e.tsv", "alone.tsv", "p_alone.tsv")}
    assert run(["--identity", paths["i.tsv"], "--parentage", paths["p.tsv"], "--cross-calls", paths["cross.vcf"],
                "--model-evidence", paths["e.tsv"]] + cross) == plain
    assert run(["--identity", paths["alone.tsv"]]) == plain                                     # stdout is unchanged
    assert open(paths["alone.tsv"]).read() == open(paths["i.tsv"]).read()
    assert run(["--parentage", paths["p_alone.tsv"]] + cross[3:]) == plain
    assert open(paths["p_alone.tsv"]).read() == open(paths["p.tsv"]).read()                     # ... and so are the other side files
    lines = open(paths["i.tsv"]).read().split("\n")
    n_records = len([ln for ln in plain.split("\n")[:-1] if not ln.startswith("#")])
    assert lines[0] == "# mchap_amd call-exact identity; frequencies: estimated; error: 0.01; records: %d; pairs not compared: 0" % n_records
    rows = [ln.split("\t") for ln in lines[2:-1]]
    assert len(rows) == 3 and all(int(r[3]) >= 2 for r in rows)
    assert [float(r[5]) for r in rows] == sorted((float(r[5]) for r in rows), reverse=True)
