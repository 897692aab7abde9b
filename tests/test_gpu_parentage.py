"""call-exact --parentage from the device: application.Parentage over the synthetic bi-parental block of
tests/test_parentage_host.py (its conditions hold here too: seed 7, six records, 60 reads a sample) against the host definition on
a float64 numpy likelihood backend, number for number after formatting; beside --cross-calls for the true pair; under a budget
that cuts the launches; and the program itself on the reference's alignment files with every other side file."""
import io as _io
import os

import numpy as np
import pytest

from tests import cross_reference as ref
from tests.test_parentage_host import BLOCK, CANDIDATES, TRUE_PROGENY, flat, ploidy_of

pytestmark = pytest.mark.gpu

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
TOL = 2e-6   # of a printed number: two values rounded to six decimals can differ by one printed unit on top of the bound


@pytest.fixture(scope="module")
def block():
    from mchap_amd import application

    records, samples, matrices, _ = ref.biparental_block(**BLOCK)
    units = application._exact_units(records, application.MatrixSource(samples, matrices), samples, None, None, False)
    return units, samples


def _rows(text):
    return [ln.split("\t") for ln in text.split("\n")[2:-1]]


def _compare(dev, host):
    """The device's table against the host's: the same lines up to TOL in LOG_BF and DELTA, the ranks equal wherever the host's
    neighbouring rows differ by more than that."""
    a, b = dev.text().split("\n"), host.text().split("\n")
    assert a[:2] == b[:2] and len(a) == len(b)
    by_key = {(r[0], r[1], r[2]): r for r in _rows(dev.text())}
    rows = _rows(host.text())
    for k, r in enumerate(rows):
        g = by_key[(r[0], r[1], r[2])]
        assert g[3:5] == r[3:5], (g, r)
        for x, y in ((g[5], r[5]), (g[6], r[6])):
            assert x == y or abs(float(x) - float(y)) <= TOL, (g, r)
        near = [o for o in rows[max(k - 1, 0):k + 2] if o is not r and o[0] == r[0] and abs(float(o[5]) - float(r[5])) <= TOL]
        if not near:
            assert g[7] == r[7], (g, r)


@pytest.mark.parametrize("inbreeding", [None, 0.1], ids=["flat", "dirmul"])
def test_the_table_against_the_host_definition(block, inbreeding):
    from mchap_amd import application

    units, samples = block
    dev = application.Parentage(samples, CANDIDATES)
    got = dev.add_block(units, ploidy_of, lambda s: inbreeding)
    host = application.Parentage(samples, CANDIDATES)
    want = host.add_block(units, ploidy_of, lambda s: inbreeding, ref.NumpyBackend())
    assert set(got) == set(want) and all((got[k] is None) == (want[k] is None) for k in want)
    _compare(dev, host)
    for c in TRUE_PROGENY:
        first = [r for r in dev.table() if r["progeny"] == c][0]
        assert (first["parent_1"], first["parent_2"], first["records"], first["skipped"]) == ("P", "Q", 6, 0)
    first = [r for r in dev.table() if r["progeny"] == "U0"][0]
    assert (first["parent_1"], first["parent_2"], first["log_bf"]) == (".", ".", 0.0)


def test_beside_the_cross_calls_of_the_true_pair(block):
    """The pair's LOG_BF is the sum of the progeny's CLBF column, which is rounded to three decimals."""
    from mchap_amd import application

    units, samples = block
    lines = ["\t".join(["chr1", str(u["rec"]["pos"]), ".", "A", ".", ".", "PASS", "AN=0", "GT"] + ["."] * len(samples)) for u in units]
    cross = application.CrossCalls(samples, ("P", "Q"), gamete_error=0.01)
    cross.add_block(units, lines, ploidy_of, flat)
    par = application.Parentage(samples, CANDIDATES, gamete_error=0.01)
    par.add_block(units, ploidy_of, flat)
    for c in TRUE_PROGENY + ("U0",):
        col = [ln.split("\t")[9 + samples.index(c)].rsplit(":", 3)[3] for ln in cross.lines]
        assert "." not in col
        row = [r for r in par.table() if (r["progeny"], r["parent_1"], r["parent_2"]) == (c, "P", "Q")][0]
        assert abs(row["log_bf"] - sum(float(x) for x in col)) <= len(col) * 5e-4


def test_a_budget_that_cuts_the_launches_gives_the_same_table(block):
    """Record by record, then progeny by progeny: equal bits -- an entry does not depend on its company --, and a budget below one
    (record, progeny) skips it and nothing else."""
    from mchap_amd import application

    units, samples = block
    whole = application.Parentage(samples, CANDIDATES)
    whole.add_block(units, ploidy_of, flat)
    need = {len(u["locus"].haplotypes): max(application._parentage_need(len(u["locus"].haplotypes), shape, 5 if shape == (2, 2) else 1)
                                            for shape in ((2, 2), (1, 3))) for u in units}
    for budget in (4 * max(need.values()), max(need.values())):        # one record a launch; one progeny a launch
        cut = application.Parentage(samples, CANDIDATES, budget=budget)
        cut.add_block(units, ploidy_of, flat)
        assert cut.skipped == whole.skipped and all(np.array_equal(cut.sums[c], whole.sums[c]) for c in whole.plan.progeny)
    small = application.Parentage(samples, CANDIDATES, budget=max(need.values()) - 1)
    small.add_block(units, ploidy_of, flat)
    big = sum(1 for u in units if need[len(u["locus"].haplotypes)] == max(need.values()))
    assert 0 < big < len(units) and all(small.skipped[c] == big and small.records[c] == len(units) - big for c in small.plan.progeny)
    host = application.Parentage(samples, CANDIDATES, budget=max(need.values()) - 1)
    host.add_block(units, ploidy_of, flat, ref.NumpyBackend())
    _compare(small, host)


def test_the_program_with_every_side_file(tmp_path):
    from mchap_amd import cli

    bams = [os.path.join(HERE, f) for f in ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")]
    base = ["mchap_amd", "call-exact", "--haplotypes", os.path.join(HERE, "mock.input.frequencies.vcf"), "--ploidy", "4", "--bam"] + bams + \
        ["--use-dirmul-prior", "0.1", "AFP", "--estimate-prior-frequencies", "3"]
    cross = ["--cross-parents", "SAMPLE1", "SAMPLE2"]
    candidates = ["--parentage-candidates", "SAMPLE1", "SAMPLE2"]

    def run(extra):
        out = _io.StringIO()
        cli.run(base + extra, out)
        return out.getvalue()

    plain = run([])
    paths = {n: str(tmp_path / n) for n in ("p.tsv", "cross.vcf", "family.vcf", "e.tsv", "snvs.vcf", "depths.vcf", "alone.tsv", "cross_alone.vcf")}
    assert run(["--parentage", paths["p.tsv"], "--cross-calls", paths["cross.vcf"], "--family-calls", paths["family.vcf"],
                "--model-evidence", paths["e.tsv"], "--snv-calls", paths["snvs.vcf"], "--allele-depths", paths["depths.vcf"]] + cross + candidates) == plain
    assert run(["--parentage", paths["alone.tsv"]] + candidates) == plain                       # stdout is unchanged
    assert open(paths["alone.tsv"]).read() == open(paths["p.tsv"]).read()
    assert run(["--cross-calls", paths["cross_alone.vcf"]] + cross) == plain
    assert open(paths["cross_alone.vcf"]).read() == open(paths["cross.vcf"]).read()             # ... and so are the other side files
    lines = open(paths["p.tsv"]).read().split("\n")
    n_records = len([ln for ln in plain.split("\n")[:-1] if not ln.startswith("#")])
    assert lines[0] == "# mchap_amd call-exact parentage; frequencies: estimated; gamete error: 0.01; records: %d" % n_records
    rows = [ln.split("\t") for ln in lines[2:-1]]
    assert len(rows) == 4 and [r[7] for r in rows] == ["1", "2", "3", "4"] and {r[0] for r in rows} == {"SAMPLE3"}
    records = [ln.split("\t") for ln in open(paths["cross.vcf"]).read().split("\n") if ln and not ln.startswith("#")]
    clbf = [r[11].rsplit(":", 3)[3] for r in records]
    pair = [r for r in rows if (r[1], r[2]) == ("SAMPLE1", "SAMPLE2")][0]
    assert int(pair[3]) >= 2
    if int(pair[4]) == 0:
        assert abs(float(pair[5]) - sum(float(x) for x in clbf if x != ".")) <= len(clbf) * 5e-4 + 1e-6
