"""call-exact --identity on the host: application.Identity over the units of a simulated panel (application.MatrixSource;
tests/identity_reference.py panel: a bi-parental family, unrelated samples of two ploidies, and one genotype filed under two
names) with a float64 numpy likelihood backend -- which pair comes first, the counting and skipping rules per pair, mixed
ploidies and mixed inbreeding, --identity-min-log-bf, the text of the table, the checks of the names.  CPU only.

Conditions of the panel (checked here on the host definition, reused by tests/test_gpu_identity.py): seed 7, six records, 60 reads
a sample -- 30 for each of the two names of P.  Under them the pair (P, P_again) scores above 20 nats and every other pair below
-10."""
import numpy as np
import pytest

from mchap_amd import application
from tests import cross_reference
from tests import identity_reference as ref


def flat(s):
    return None


@pytest.fixture(scope="module")
def block():
    records, samples, matrices, ploidy_of = ref.panel()
    units = application._exact_units(records, application.MatrixSource(samples, matrices), samples, None, None, False)
    return units, samples, ploidy_of


@pytest.fixture(scope="module")
def table(block):
    units, samples, ploidy_of = block
    tab = application.Identity(samples)
    tab.add_block(units, ploidy_of, flat, cross_reference.NumpyBackend())
    return tab


def test_the_pairs_of_the_panel(table, capsys):
    plan = table.plan
    assert plan.samples == ["P", "Q", "C0", "C1", "C2", "U0", "X0", "X2", "X3", "P_again"]
    assert list(plan.classes) == [(4, None), (2, None)] and plan.classes[(2, None)] == ["X2", "X3"]
    assert len(plan.pairs) == 28 + 1 and plan.not_compared == 16 and plan.pairs[0] == ("P", "Q") and plan.pairs[-1] == ("X2", "X3")
    assert ("X0", "P_again") in plan.pairs and ("P_again", "X0") not in plan.pairs      # SAMPLE_1 before SAMPLE_2 in sample order
    application.Identity(["A", "B", "D"]).resolve(lambda s: 2 if s == "D" else 4, flat)
    assert "2 pairs of samples differ in ploidy or inbreeding and are not compared" in capsys.readouterr().err


def test_the_two_names_of_one_genotype_come_first(table):
    rows = table.table()
    assert (rows[0]["sample_1"], rows[0]["sample_2"]) == ref.DUPLICATE and rows[0]["log_bf"] > 20.0
    assert all(r["log_bf"] < -10.0 for r in rows[1:]) and len(rows) == 29
    assert all(a["log_bf"] >= b["log_bf"] for a, b in zip(rows, rows[1:]))
    assert all(r["records"] == 6 and r["skipped"] == 0 for r in rows)
    assert {r["ploidy"] for r in rows} == {2, 4} and [r["ploidy"] for r in rows if r["sample_1"] == "X2"] == [2]
    # a term is bounded below by log e: six records
    assert min(r["log_bf"] for r in rows) >= 6 * np.log(0.01) - 1e-9


def test_a_term_is_the_unit_definition(block, table):
    units, samples, ploidy_of = block
    got = application.identity_host(units, samples, ploidy_of, flat, table.plan, 0.01, cross_reference.NumpyBackend())
    names = table.plan.classes[(4, None)]
    i, j = names.index("P"), names.index("P_again")
    total = 0.0
    for ri, unit in enumerate(units):
        H = len(unit["locus"].haplotypes)
        llk = np.stack([application._unit_llk(unit, s, 4, cross_reference.NumpyBackend()) for s in ("P", "P_again")])
        want = application.identity_unit(llk, ref.log_prior(4, H, None, None), 0.01)[0, 1]
        assert got[(ri, (4, None))][i, j] == pytest.approx(want, rel=1e-12, abs=1e-12)
        total = total + got[(ri, (4, None))][i, j]
    assert table.sums[ref.DUPLICATE] == total


class Poisoned:
    """The numpy backend, with the likelihoods of chosen read tensors all minus infinity: a sample without a finite genotype."""

    def __init__(self, tensors):
        self.tensors, self.inner = tensors, cross_reference.NumpyBackend()

    def genotype_likelihoods(self, dists, ploidy, haplotypes, read_counts=None):
        llk = self.inner.genotype_likelihoods(dists, ploidy, haplotypes, read_counts=read_counts)
        return np.full(len(llk), -np.inf) if any(dists is t for t in self.tensors) else llk


def test_skipping_is_per_pair(block, table):
    units, samples, ploidy_of = block
    tab = application.Identity(samples)
    tab.add_block(units, ploidy_of, flat, Poisoned([units[2]["reads"]["Q"]["dists"]]))
    for pair in tab.plan.pairs:
        with_q = "Q" in pair
        assert (tab.records[pair], tab.skipped[pair]) == ((5, 1) if with_q else (6, 0))
        if not with_q:
            assert tab.sums[pair] == table.sums[pair]
    rest = application.Identity(samples)
    rest.add_block([u for i, u in enumerate(units) if i != 2], ploidy_of, flat, cross_reference.NumpyBackend())
    assert tab.sums[("P", "Q")] == rest.sums[("P", "Q")] and tab.sums[("Q", "P_again")] == rest.sums[("Q", "P_again")]


def test_a_sample_without_reads_adds_exactly_zero(block, table):
    units, samples, ploidy_of = block
    bare = [dict(u) for u in units]
    bare[3] = dict(bare[3], reads=dict(bare[3]["reads"]))
    sr = bare[3]["reads"]["C2"]
    bare[3]["reads"]["C2"] = dict(dists=sr["dists"][:0], counts=sr["counts"][:0])
    tab = application.Identity(samples)
    got = tab.add_block(bare, ploidy_of, flat, cross_reference.NumpyBackend())
    at = tab.plan.classes[(4, None)].index("C2")
    row = got[(3, (4, None))][at]
    assert np.all(row[np.arange(len(row)) != at] == 0.0)
    rest = application.Identity(samples)
    rest.add_block([u for i, u in enumerate(units) if i != 3], ploidy_of, flat, cross_reference.NumpyBackend())
    for pair in tab.plan.pairs:
        assert (tab.records[pair], tab.skipped[pair]) == (6, 0)
        assert tab.sums[pair] == (rest.sums[pair] if "C2" in pair else table.sums[pair])


def test_a_record_with_a_single_haplotype_is_counted_and_adds_nothing(block, table):
    units, samples, ploidy_of = block
    one = dict(units[0], needs_kernel=False, locus=type("L", (), dict(haplotypes=units[0]["locus"].haplotypes[:1], frequencies=np.ones(1)))())
    tab = application.Identity(samples)
    tab.add_block(list(units) + [one, dict(units[1], needs_kernel=False, invalid="AF0")], ploidy_of, flat, cross_reference.NumpyBackend())
    assert tab.records_seen == 8 and all(tab.records[p] == 7 and tab.skipped[p] == 0 for p in tab.plan.pairs)
    assert tab.sums == table.sums


def test_a_refused_shape_and_a_small_budget_skip_the_record_for_the_class(block, table):
    units, samples, ploidy_of = block
    # the tetraploid class of a record of five haplotypes: 70 genotypes, ten samples
    need = {H: application._identity_need(H, 4, 10) for H in (3, 4, 5)}
    assert need[3] < need[4] < need[5]
    tab = application.Identity(samples, budget=need[4])
    tab.add_block(units, ploidy_of, flat, cross_reference.NumpyBackend())
    five = sum(1 for u in units if len(u["locus"].haplotypes) == 5)
    assert five == 2
    for pair in tab.plan.pairs:
        tetra = tab.plan.key[pair[0]][0] == 4
        assert (tab.records[pair], tab.skipped[pair]) == ((6 - five, five) if tetra else (6, 0))
    assert tab.sums[("X2", "X3")] == table.sums[("X2", "X3")]
    # a ploidy beyond the library's: every record of the class is skipped, nothing is raised
    tab = application.Identity(samples, names=["X2", "X3"])
    tab.add_block(units, lambda s: 16, flat, cross_reference.NumpyBackend())
    assert tab.records[("X2", "X3")] == 0 and tab.skipped[("X2", "X3")] == 6


def test_mixed_inbreeding_and_chosen_samples(block, table, capsys):
    units, samples, ploidy_of = block
    inbreeding = lambda s: 0.3 if s in ("Q", "C0") else 0.1     # noqa: E731
    tab = application.Identity(samples, names=["C0", "P_again", "Q", "P", "X2"])
    tab.add_block(units, ploidy_of, inbreeding, cross_reference.NumpyBackend())
    assert "8 pairs of samples differ in ploidy or inbreeding" in capsys.readouterr().err
    assert tab.plan.samples == ["P", "Q", "C0", "X2", "P_again"] and tab.plan.pairs == [("P", "P_again"), ("Q", "C0")]
    rows = tab.table()
    assert [(r["sample_1"], r["sample_2"]) for r in rows] == [("P", "P_again"), ("Q", "C0")] and rows[0]["log_bf"] > 20.0
    assert "pairs not compared: 8" in tab.text().split("\n")[0]
    assert application.Identity(samples, names=["P", "P_again"], min_log_bf=0.0).min_log_bf == 0.0


def test_min_log_bf_keeps_the_rows_at_or_above_it(block, table):
    units, samples, ploidy_of = block
    tab = application.Identity(samples, min_log_bf=-12.0)
    tab.add_block(units, ploidy_of, flat, cross_reference.NumpyBackend())
    full = table.table()
    assert tab.table() == [r for r in full if r["log_bf"] >= -12.0] and len(tab.table()) == 2
    edge = application.Identity(samples, min_log_bf=full[1]["log_bf"])
    edge.add_block(units, ploidy_of, flat, cross_reference.NumpyBackend())
    assert len(edge.table()) == 2


def test_the_text_character_for_character():
    samples = ["A", "B", "K", "D"]
    tab = application.Identity(samples, error=0.0, frequency_source="tag AFP")
    tab.resolve(lambda s: 2 if s == "D" else 4, flat)
    assert tab.plan.pairs == [("A", "B"), ("A", "K"), ("B", "K")]
    tab.sums = {("A", "B"): -np.inf, ("A", "K"): 12.3456789, ("B", "K"): 12.3456789}
    tab.records, tab.skipped, tab.records_seen = {("A", "B"): 7, ("A", "K"): 5, ("B", "K"): 6}, {("A", "B"): 0, ("A", "K"): 2, ("B", "K"): 1}, 7
    assert tab.text() == ("# mchap_amd call-exact identity; frequencies: tag AFP; error: 0; records: 7; pairs not compared: 3\n"
                          "SAMPLE_1\tSAMPLE_2\tPLOIDY\tRECORDS\tSKIPPED\tLOG_BF\n"
                          "A\tK\t4\t5\t2\t12.345679\n"          # a tie: in pair order, by i then j
                          "B\tK\t4\t6\t1\t12.345679\n"
                          "A\tB\t4\t7\t0\t-inf\n")
    tab.min_log_bf = 0.0
    assert len(tab.text().split("\n")) == 5


@pytest.mark.parametrize("kw, text", [
    (dict(names=["A", "Z"]), "is not a sample"),
    (dict(names=["A", "A"]), "more than once"),
    (dict(names=["A"]), "at least two samples"),
    (dict(names=[]), "at least two samples"),
    (dict(error=1.5), r"error lies in \[0, 1\]"),
    (dict(error=-0.1), r"error lies in \[0, 1\]"),
    (dict(error=float("nan")), r"error lies in \[0, 1\]"),
    (dict(min_log_bf=float("nan")), "is a number"),
])
def test_the_checks_of_the_names(kw, text):
    with pytest.raises(ValueError, match=text):
        application.Identity(["A", "B", "K"], **kw).resolve(lambda s: 4, flat)


def test_one_sample_alone_in_the_run():
    with pytest.raises(ValueError, match="at least two samples"):
        application.Identity(["A"]).resolve(lambda s: 4, flat)
