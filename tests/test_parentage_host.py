"""call-exact --parentage on the host: application.Parentage over the units of a synthetic bi-parental block
(application.MatrixSource; tests/cross_reference.py biparental_block with extra, unrelated candidates) with a float64 numpy
likelihood backend -- which pair comes first, the unknown pair's exact 0, the counting and skipping rules, a sample that is a
candidate and a progeny, --parentage-top, the text of the table, the checks of the hypotheses.  CPU only.

Conditions of the block (checked here on the host definition, reused by tests/test_gpu_parentage.py): seed 7, six records, 60
reads a sample, the candidates P, X0, Q, X1 (tetraploid) and X2 (diploid).  Under them the true pair (P, Q) is the first row of
every true progeny by more than 3 nats, and the unrelated sample's first row is the unknown pair."""
import numpy as np
import pytest

from mchap_amd import application
from tests import cross_reference as ref

EXTRA = {"X0": 4, "X1": 4, "X2": 2}
CANDIDATES = ["P", "X0", "Q", "X1", "X2"]
BLOCK = dict(seed=7, n_records=6, depth=60, extra=EXTRA)
TRUE_PROGENY = ("C0", "C1", "C2")


def ploidy_of(s):
    return EXTRA.get(s, 4)


def flat(s):
    return None


@pytest.fixture(scope="module")
def block():
    records, samples, matrices, truth = ref.biparental_block(**BLOCK)
    units = application._exact_units(records, application.MatrixSource(samples, matrices), samples, None, None, False)
    return units, samples


@pytest.fixture(scope="module")
def table(block):
    units, samples = block
    par = application.Parentage(samples, CANDIDATES)
    par.add_block(units, ploidy_of, flat, ref.NumpyBackend())
    return par


def rows_of(par, c):
    return [r for r in par.table() if r["progeny"] == c]


def test_the_hypotheses_of_the_block(table):
    plan = table.plan
    assert plan.progeny == ["C0", "C1", "C2", "U0"]                                  # every sample that is not a candidate
    pairs = [("P", "X0"), ("P", "Q"), ("P", "X1"), ("X0", "Q"), ("X0", "X1"), ("Q", "X1")]   # i < j in candidate order, 2 + 2 = 4
    single = [(s, ".") for s in CANDIDATES]                                         # X2 with the population's gamete of three
    assert plan.hypotheses["C0"] == pairs + single + [(".", ".")]
    assert plan.launches[4] == [(2, 2), (1, 3)]
    assert plan.where("C0", ("X2", ".")) == ((1, 3), 0, 0) and plan.where("C0", ("Q", ".")) == ((2, 2), 2, 4)


def test_the_true_pair_comes_first_and_the_unrelated_sample_fits_nobody(table):
    for c in TRUE_PROGENY:
        rows = rows_of(table, c)
        assert (rows[0]["parent_1"], rows[0]["parent_2"]) == ("P", "Q") and rows[0]["delta"] == 0.0 and rows[0]["rank"] == 1
        assert rows[1]["delta"] < -3.0 and rows[0]["log_bf"] > 3.0
        assert [r["rank"] for r in rows] == list(range(1, 13)) and all(a["log_bf"] >= b["log_bf"] for a, b in zip(rows, rows[1:]))
        assert all(r["records"] == 6 and r["skipped"] == 0 for r in rows)
    rows = rows_of(table, "U0")
    assert (rows[0]["parent_1"], rows[0]["parent_2"]) == (".", ".") and rows[1]["delta"] < -3.0


def test_the_unknown_pair_is_exactly_zero(table):
    for c in table.plan.progeny:
        null = [r for r in rows_of(table, c) if (r["parent_1"], r["parent_2"]) == (".", ".")]
        assert len(null) == 1 and null[0]["log_bf"] == 0.0


def test_the_pair_is_the_cross_calls_log_bayes_factor(block, table):
    """For the pair (P, Q) a record's term is the CLBF of --cross-calls --cross-parents P Q at the same gamete error."""
    units, samples = block
    cross = application.Cross(("P", "Q"), ["C0", "C1", "C2", "U0"], 0.01)
    calls = application.cross_calls_host(units, samples, ploidy_of, flat, cross, ref.NumpyBackend())
    got = application.parentage_host(units, samples, ploidy_of, flat, table.plan, 0.01, ref.NumpyBackend())
    k = table.plan.hypotheses["C0"].index(("P", "Q"))
    for (ri, c), call in calls.items():
        assert got[(ri, c)][k] == pytest.approx(call[2], rel=1e-9, abs=1e-12)


class Poisoned:
    """The numpy backend, with the likelihoods of chosen read tensors all minus infinity: a sample without a finite genotype."""

    def __init__(self, tensors):
        self.tensors, self.inner = tensors, ref.NumpyBackend()

    def genotype_likelihoods(self, dists, ploidy, haplotypes, read_counts=None):
        llk = self.inner.genotype_likelihoods(dists, ploidy, haplotypes, read_counts=read_counts)
        return np.full(len(llk), -np.inf) if any(dists is t for t in self.tensors) else llk


def test_a_candidate_without_a_finite_genotype_is_skipped_where_it_could_be_a_parent(block, table):
    units, samples = block
    # X2 is a progeny too: a diploid whose one gamete X0 (two haplotypes a gamete) cannot have given
    par = application.Parentage(samples, CANDIDATES, ["C0", "C1", "C2", "U0", "X2"])
    par.add_block(units, ploidy_of, flat, Poisoned([units[2]["reads"]["X0"]["dists"]]))
    for c in ("C0", "C1", "C2", "U0"):
        assert par.records[c] == 5 and par.skipped[c] == 1
    assert par.records["X2"] == 6 and par.skipped["X2"] == 0
    # ... and the record is left out of EVERY row, the rows without X0 too: the other five records' sums
    units5 = [u for i, u in enumerate(units) if i != 2]
    rest = application.Parentage(samples, CANDIDATES, ["C0", "C1", "C2", "U0", "X2"])
    rest.add_block(units5, ploidy_of, flat, ref.NumpyBackend())
    for c in par.plan.progeny:
        assert np.array_equal(par.sums[c], rest.sums[c])
    # a progeny without a finite genotype is skipped itself, and nobody else
    par = application.Parentage(samples, CANDIDATES)
    par.add_block(units, ploidy_of, flat, Poisoned([units[4]["reads"]["C1"]["dists"]]))
    assert par.skipped == {"C0": 0, "C1": 1, "C2": 0, "U0": 0} and par.records["C1"] == 5


def test_a_progeny_without_reads_adds_exactly_zero(block, table):
    units, samples = block
    bare = [dict(u) for u in units]
    bare[3] = dict(bare[3], reads=dict(bare[3]["reads"]))
    sr = bare[3]["reads"]["C2"]
    bare[3]["reads"]["C2"] = dict(dists=sr["dists"][:0], counts=sr["counts"][:0])
    par = application.Parentage(samples, CANDIDATES)
    got = par.add_block(bare, ploidy_of, flat, ref.NumpyBackend())
    assert np.array_equal(got[(3, "C2")], np.zeros(12)) and par.records["C2"] == 6 and par.skipped["C2"] == 0
    rest = application.Parentage(samples, CANDIDATES)
    rest.add_block([u for i, u in enumerate(units) if i != 3], ploidy_of, flat, ref.NumpyBackend())
    assert np.array_equal(par.sums["C2"], rest.sums["C2"])
    assert np.array_equal(par.sums["C0"], table.sums["C0"])


def test_a_sample_that_is_candidate_and_progeny(block):
    units, samples = block
    par = application.Parentage(samples, CANDIDATES + ["C0"], ["C0", "C1", "U0"])
    par.add_block(units, ploidy_of, flat, ref.NumpyBackend())
    assert all("C0" not in row for row in par.plan.hypotheses["C0"])
    assert ("P", "C0") in par.plan.hypotheses["C1"] and ("C0", ".") in par.plan.hypotheses["C1"]
    rows = rows_of(par, "C0")
    assert (rows[0]["parent_1"], rows[0]["parent_2"]) == ("P", "Q") and len(rows) == 12
    assert len(rows_of(par, "C1")) == 10 + 6 + 1


def test_top_keeps_the_first_rows(block, table):
    units, samples = block
    par = application.Parentage(samples, CANDIDATES, top=2)
    par.add_block(units, ploidy_of, flat, ref.NumpyBackend())
    full = table.table()
    assert par.table() == [r for r in full if r["rank"] <= 2] and len(par.table()) == 8


def test_a_record_with_a_single_haplotype_is_counted_and_adds_nothing(block, table):
    units, samples = block
    one = dict(units[0], needs_kernel=False, locus=type("L", (), dict(haplotypes=units[0]["locus"].haplotypes[:1], frequencies=np.ones(1)))())
    par = application.Parentage(samples, CANDIDATES)
    par.add_block(list(units) + [one, dict(units[1], needs_kernel=False, invalid="AF0")], ploidy_of, flat, ref.NumpyBackend())
    assert par.records_seen == 8 and all(par.records[c] == 7 and par.skipped[c] == 0 for c in par.plan.progeny)
    assert all(np.array_equal(par.sums[c], table.sums[c]) for c in par.plan.progeny)


def test_the_text_character_for_character():
    samples = ["A", "B", "K", "D"]
    par = application.Parentage(samples, ["A", "B"], gamete_error=0.0, frequency_source="tag AFP")
    par.resolve(lambda s: 2 if s == "D" else 4)
    assert par.plan.hypotheses == {"K": [("A", "B"), ("A", "."), ("B", "."), (".", ".")], "D": [(".", ".")]}
    par.sums["K"] = np.array([12.3456789, -np.inf, 12.3456789, 0.0])
    par.records, par.skipped, par.records_seen = {"K": 5, "D": 6}, {"K": 1, "D": 0}, 7
    assert par.text() == ("# mchap_amd call-exact parentage; frequencies: tag AFP; gamete error: 0; records: 7\n"
                          "PROGENY\tPARENT_1\tPARENT_2\tRECORDS\tSKIPPED\tLOG_BF\tDELTA\tRANK\n"
                          "K\tA\tB\t5\t1\t12.345679\t0.000000\t1\n"
                          "K\tB\t.\t5\t1\t12.345679\t0.000000\t2\n"
                          "K\t.\t.\t5\t1\t0.000000\t-12.345679\t3\n"
                          "K\tA\t.\t5\t1\t-inf\t-inf\t4\n"
                          "D\t.\t.\t6\t0\t0.000000\t0.000000\t1\n")


def test_a_progeny_nobody_fits_is_named_on_stderr(capsys):
    par = application.Parentage(["A", "B", "D"], ["A", "B"])
    par.resolve(lambda s: 2 if s == "D" else 4)
    assert "no candidate fits progeny D" in capsys.readouterr().err


@pytest.mark.parametrize("kw, text", [
    (dict(candidates=["A", "Z"]), "is not a sample"),
    (dict(candidates=["A", "A"]), "more than once"),
    (dict(candidates=["A", "B"], progeny=["K", "K"]), "more than once"),
    (dict(candidates=["A", "B"], progeny=["Y"]), "is not a sample"),
    (dict(candidates=["A", "O"]), "even ploidy"),
    (dict(candidates=["A"], gamete_error=1.5), "gamete error"),
    (dict(candidates=["A"], gamete_error=float("nan")), "gamete error"),
    (dict(candidates=["A"], top=-1), "0 (all) or more"),
    (dict(candidates=[]), "no candidate"),
])
def test_the_checks_of_the_hypotheses(kw, text):
    with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
        application.Parentage(["A", "B", "K", "O"], **kw).resolve(lambda s: 3 if s == "O" else 4)
