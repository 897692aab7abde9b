"""call-exact --parentage --parentage-selfings on the host: application.Parentage(..., selfings=True) over the units of a synthetic
block with a selfed progeny (application.MatrixSource; tests/selfing_reference.py selfing_block) with a float64 numpy likelihood
backend -- the order of the rows, who ranks first, the selfing rows at a gamete error of 1, the counting and skipping rules with
selfings on, and that nothing moves with selfings off.  CPU only.

Conditions of the block (picked on the host definition, reused by tests/test_gpu_parentage_selfings.py): seed 11, six records, 40
reads a sample, tetraploid throughout, the candidates P and Q; S0 a true self of P, C0 a true P x Q progeny, D0 a duplicate of P.
Under them S0 ranks (P, P) first (LOG_BF 10.4) with (P, .) 6.6 nats and (P, Q) 21 nats behind; C0 still ranks (P, Q) first; the
duplicate D0 -- P's own genotype is one a self of P can have -- ranks (P, P) first too."""
import numpy as np
import pytest

from mchap_amd import application
from tests import selfing_reference as ref
from tests.cross_reference import NumpyBackend
from tests.test_parentage_host import Poisoned

BLOCK = dict(seed=11, n_records=6, depth=40)
CANDIDATES = ["P", "Q"]


def ploidy_of(s):
    return 4


def flat(s):
    return None


@pytest.fixture(scope="module")
def block():
    records, samples, matrices, truth = ref.selfing_block(**BLOCK)
    units = application._exact_units(records, application.MatrixSource(samples, matrices), samples, None, None, False)
    return units, samples


@pytest.fixture(scope="module")
def table(block):
    units, samples = block
    par = application.Parentage(samples, CANDIDATES, selfings=True)
    par.add_block(units, ploidy_of, flat, NumpyBackend())
    return par


def rows_of(par, c):
    return [r for r in par.table() if r["progeny"] == c]


def test_the_rows_and_their_order():
    samples = ["A", "B", "X", "K", "D"]
    of = lambda s: {"X": 2, "D": 2}.get(s, 4)   # noqa: E731
    plan = application.ParentagePlan(samples, ["A", "B", "X"], ["A", "K", "D"], of, selfings=True)
    # pairs, selfings in candidate order, (i, .), (., .); X (diploid) selfed would give a diploid: a row of D alone
    assert plan.hypotheses["K"] == [("A", "B"), ("A", "A"), ("B", "B"), ("A", "."), ("B", "."), ("X", "."), (".", ".")]
    assert plan.hypotheses["A"] == [("B", "B"), ("B", "."), ("X", "."), (".", ".")]            # the progeny itself is left out
    assert plan.hypotheses["D"] == [("X", "X"), ("X", "."), (".", ".")]                        # a ploidy mismatch gives no row
    assert plan.selfed == {4: ["A", "B"], 2: ["X"]} and plan.selfs("K") == ["A", "B"] and plan.selfs("A") == ["B"]
    assert plan.used("A") == ["B", "X"] and plan.used("D") == ["X"]
    assert plan.launches[4] == [(2, 2), (1, 3)] and plan.launches[2] == [(1, 1)]               # no parentage launch for a selfing
    off = application.ParentagePlan(samples, ["A", "B", "X"], ["A", "K", "D"], of)
    assert off.hypotheses["K"] == [("A", "B"), ("A", "."), ("B", "."), ("X", "."), (".", ".")] and off.selfed == {} and not off.selfings
    assert off.launches == plan.launches


def test_with_selfings_off_nothing_moves(block):
    units, samples = block
    a, b = application.Parentage(samples, CANDIDATES), application.Parentage(samples, CANDIDATES, selfings=False)
    a.add_block(units, ploidy_of, flat, NumpyBackend())
    b.add_block(units, ploidy_of, flat, NumpyBackend())
    assert a.text() == b.text() and "selfings" not in a.text() and a.plan.hypotheses == b.plan.hypotheses
    assert all(("P", "P") not in rows for rows in a.plan.hypotheses.values())
    with pytest.raises(ValueError, match="without selfings"):
        application.parentage_host(units, samples, ploidy_of, flat, a.plan, 0.01, NumpyBackend(), selfings=True)


def test_the_self_ranks_first_and_the_cross_still_does(table):
    rows = rows_of(table, "S0")
    by = {(r["parent_1"], r["parent_2"]): r for r in rows}
    assert (rows[0]["parent_1"], rows[0]["parent_2"]) == ("P", "P") and rows[0]["rank"] == 1 and rows[0]["log_bf"] > 3.0
    assert by[("P", "Q")]["delta"] <= -3.0 and by[("P", ".")]["delta"] <= -3.0
    assert all(r["records"] == 6 and r["skipped"] == 0 for r in rows) and len(rows) == 6
    rows = rows_of(table, "C0")
    assert (rows[0]["parent_1"], rows[0]["parent_2"]) == ("P", "Q")
    rows = rows_of(table, "D0")
    assert (rows[0]["parent_1"], rows[0]["parent_2"]) == ("P", "P")
    assert "; selfings: yes\n" in table.text() and "\nS0\tP\tP\t6\t0\t" in table.text()


def test_the_other_rows_are_the_table_without_selfings(block, table):
    units, samples = block
    off = application.Parentage(samples, CANDIDATES)
    off.add_block(units, ploidy_of, flat, NumpyBackend())
    for c in table.plan.progeny:
        keep = [k for k, (p, q) in enumerate(table.plan.hypotheses[c]) if p != q or p == "."]
        assert np.array_equal(table.sums[c][keep], off.sums[c])


def test_a_selfing_row_is_the_unit_definition(block, table):
    units, samples = block
    got = application.parentage_host(units, samples, ploidy_of, flat, table.plan, 0.01, NumpyBackend(), selfings=True)
    k = table.plan.hypotheses["S0"].index(("P", "P"))
    backend = NumpyBackend()
    for ri, unit in enumerate(units):
        H, f = len(unit["locus"].haplotypes), unit["locus"].frequencies
        llk_c = application._unit_llk(unit, "S0", 4, backend)
        out = application.selfing_prior_unit(application._unit_llk(unit, "P", 4, backend), 4, None, H, f, 0.01, llk_c)
        norm = application._unit_posterior(llk_c, H, 4, None, f)[1]
        assert got[(ri, "S0")][k] == pytest.approx(out["log_z"] - norm, rel=1e-12, abs=1e-12)


def test_at_a_gamete_error_of_one_a_selfing_row_is_zero(block):
    """e = 1: S is the population's multinomial Mult(gc; K, f).  With F = 0 the progeny's calling prior IS that multinomial, so a
    record's term log_z - log Z_pop is 0 but for the rounding of its two operands: per record |term| <= REL (|log_z| + |log Z_pop|) +
    FLOOR, each operand held as every log evidence here is."""
    units, samples = block
    backend = NumpyBackend()
    plan = application.ParentagePlan(samples, CANDIDATES, None, ploidy_of, selfings=True)
    got = application.parentage_host(units, samples, ploidy_of, lambda s: 0.0, plan, 1.0, backend, selfings=True)
    for c in plan.progeny:
        for k, (p, q) in enumerate(plan.hypotheses[c]):
            if p != q or p == ".":
                continue
            for ri, unit in enumerate(units):
                H, f = len(unit["locus"].haplotypes), unit["locus"].frequencies
                llk_c = application._unit_llk(unit, c, 4, backend)
                log_z = application.selfing_prior_unit(application._unit_llk(unit, p, 4, backend), 4, 0.0, H, f, 1.0, llk_c)["log_z"]
                norm = application._unit_posterior(llk_c, H, 4, 0.0, f)[1]
                assert abs(got[(ri, c)][k]) <= ref.REL * (abs(log_z) + abs(norm)) + ref.FLOOR, (c, p, ri, got[(ri, c)][k])


def test_the_skipping_rules_hold_with_selfings_on(block, table):
    units, samples = block
    # a candidate without a finite genotype: the record is left out of EVERY row of the progeny it could have given
    par = application.Parentage(samples, CANDIDATES, selfings=True)
    par.add_block(units, ploidy_of, flat, Poisoned([units[2]["reads"]["P"]["dists"]]))
    rest = application.Parentage(samples, CANDIDATES, selfings=True)
    rest.add_block([u for i, u in enumerate(units) if i != 2], ploidy_of, flat, NumpyBackend())
    for c in par.plan.progeny:
        assert par.records[c] == 5 and par.skipped[c] == 1 and np.array_equal(par.sums[c], rest.sums[c])
    # a progeny without a finite genotype is skipped itself, and nobody else
    par = application.Parentage(samples, CANDIDATES, selfings=True)
    par.add_block(units, ploidy_of, flat, Poisoned([units[4]["reads"]["S0"]["dists"]]))
    assert par.skipped == {"S0": 1, "C0": 0, "D0": 0} and par.records["S0"] == 5
    # a progeny without reads adds exactly 0 to every row, the selfing rows too
    bare = [dict(u) for u in units]
    bare[3] = dict(bare[3], reads=dict(bare[3]["reads"]))
    sr = bare[3]["reads"]["S0"]
    bare[3]["reads"]["S0"] = dict(dists=sr["dists"][:0], counts=sr["counts"][:0])
    par = application.Parentage(samples, CANDIDATES, selfings=True)
    got = par.add_block(bare, ploidy_of, flat, NumpyBackend())
    assert np.array_equal(got[(3, "S0")], np.zeros(6)) and par.records["S0"] == 6 and par.skipped["S0"] == 0
    # a sample that is candidate and progeny: never its own self
    par = application.Parentage(samples, CANDIDATES + ["D0"], ["S0", "D0"], selfings=True)
    par.add_block(units, ploidy_of, flat, NumpyBackend())
    assert ("D0", "D0") not in par.plan.hypotheses["D0"] and ("D0", "D0") in par.plan.hypotheses["S0"]
    # a launch beyond the budget skips the (record, progeny) in all its rows
    par = application.Parentage(samples, CANDIDATES, selfings=True, budget=64)
    par.add_block(units, ploidy_of, flat, NumpyBackend())
    assert all(par.skipped[c] == 6 and par.records[c] == 0 for c in par.plan.progeny)
    # a record with a single haplotype is counted and adds nothing
    one = dict(units[0], needs_kernel=False, locus=type("L", (), dict(haplotypes=units[0]["locus"].haplotypes[:1], frequencies=np.ones(1)))())
    par = application.Parentage(samples, CANDIDATES, selfings=True)
    par.add_block(list(units) + [one], ploidy_of, flat, NumpyBackend())
    assert all(par.records[c] == 7 and np.array_equal(par.sums[c], table.sums[c]) for c in par.plan.progeny)


def test_the_text_character_for_character():
    par = application.Parentage(["A", "B", "K"], ["A", "B"], gamete_error=0.0, selfings=True)
    par.resolve(lambda s: 4)
    assert par.plan.hypotheses == {"K": [("A", "B"), ("A", "A"), ("B", "B"), ("A", "."), ("B", "."), (".", ".")]}
    par.sums["K"] = np.array([1.5, 12.3456789, -np.inf, 2.0, 12.3456789, 0.0])
    par.records, par.skipped, par.records_seen = {"K": 5}, {"K": 1}, 7
    assert par.text() == ("# mchap_amd call-exact parentage; frequencies: flat; gamete error: 0; records: 7; selfings: yes\n"
                          "PROGENY\tPARENT_1\tPARENT_2\tRECORDS\tSKIPPED\tLOG_BF\tDELTA\tRANK\n"
                          "K\tA\tA\t5\t1\t12.345679\t0.000000\t1\n"
                          "K\tB\t.\t5\t1\t12.345679\t0.000000\t2\n"
                          "K\tA\t.\t5\t1\t2.000000\t-10.345679\t3\n"
                          "K\tA\tB\t5\t1\t1.500000\t-10.845679\t4\n"
                          "K\t.\t.\t5\t1\t0.000000\t-12.345679\t5\n"
                          "K\tB\tB\t5\t1\t-inf\t-inf\t6\n")


def test_the_ranking_holds_on_the_oracle_backend(block):
    """The same conditions with the CPU oracle's likelihoods (float32, as the reference's) in place of the numpy backend's."""
    from tests.replay_call_exact import OracleBackend

    units, samples = block
    par = application.Parentage(samples, CANDIDATES, selfings=True)
    par.add_block(units, ploidy_of, flat, OracleBackend())
    rows = rows_of(par, "S0")
    by = {(r["parent_1"], r["parent_2"]): r for r in rows}
    assert (rows[0]["parent_1"], rows[0]["parent_2"]) == ("P", "P") and by[("P", "Q")]["delta"] <= -3.0 and by[("P", ".")]["delta"] <= -3.0
    rows = rows_of(par, "C0")
    assert (rows[0]["parent_1"], rows[0]["parent_2"]) == ("P", "Q")
