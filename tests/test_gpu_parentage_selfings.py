"""call-exact --parentage --parentage-selfings from the device: application.Parentage(..., selfings=True) over the block of
tests/test_parentage_selfings_host.py (its conditions hold here too: seed 11, six records, 40 reads a sample) against the host
definition on a float64 numpy likelihood backend -- order and SKIPPED equal, LOG_BF within the records times (1e-9 |want| + 8 x
ENVELOPE) --; under a budget that cuts the launches; and with selfings off against the host table without selfings."""
import numpy as np
import pytest

from tests import selfing_reference as ref
from tests.cross_reference import NumpyBackend
from tests.test_gpu_parentage import _compare
from tests.test_parentage_selfings_host import BLOCK, CANDIDATES, flat, ploidy_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def block():
    from mchap_amd import application

    records, samples, matrices, _ = ref.selfing_block(**BLOCK)
    units = application._exact_units(records, application.MatrixSource(samples, matrices), samples, None, None, False)
    return units, samples


def _hold(dev, host, n_records):
    assert dev.plan.hypotheses == host.plan.hypotheses and dev.skipped == host.skipped and dev.records == host.records
    worst = 0.0
    for c in host.plan.progeny:
        want, got = host.sums[c], dev.sums[c]
        err = np.abs(got - want)
        print(c, "largest |device - host| of a LOG_BF %.3g" % err.max(), "host", np.round(want, 3))
        assert np.all(err <= n_records * (ref.REL * np.abs(want) + ref.FLOOR)), (c, got, want)
        worst = max(worst, float(err.max()))
    a, b = [(r["progeny"], r["parent_1"], r["parent_2"]) for r in dev.table()], [(r["progeny"], r["parent_1"], r["parent_2"]) for r in host.table()]
    assert a == b                                                       # the order of the rows
    return worst


@pytest.mark.parametrize("inbreeding", [None, 0.1], ids=["flat", "dirmul"])
def test_the_table_against_the_host_definition(block, inbreeding):
    from mchap_amd import application

    units, samples = block
    dev = application.Parentage(samples, CANDIDATES, selfings=True)
    got = dev.add_block(units, ploidy_of, lambda s: inbreeding)
    host = application.Parentage(samples, CANDIDATES, selfings=True)
    want = host.add_block(units, ploidy_of, lambda s: inbreeding, NumpyBackend())
    assert set(got) == set(want) and all((got[k] is None) == (want[k] is None) for k in want)
    _hold(dev, host, len(units))
    first = [r for r in dev.table() if r["progeny"] == "S0"][0]
    assert (first["parent_1"], first["parent_2"], first["records"], first["skipped"]) == ("P", "P", 6, 0)
    first = [r for r in dev.table() if r["progeny"] == "C0"][0]
    assert (first["parent_1"], first["parent_2"]) == ("P", "Q")
    assert dev.text().split("\n")[0].endswith("; selfings: yes")


def test_a_budget_that_cuts_the_launches_gives_the_same_table(block):
    """Record by record, then progeny by progeny, the selfing-prior launch unit by unit: equal bits -- an entry does not depend on
    its company --, and a budget below one (record, progeny) skips it and nothing else."""
    from mchap_amd import application

    units, samples = block
    whole = application.Parentage(samples, CANDIDATES, selfings=True)
    whole.add_block(units, ploidy_of, flat)
    need = {}
    for u in units:
        H = len(u["locus"].haplotypes)
        need[H] = max([application._parentage_need(H, (2, 2), 3)] + list(application._selfing_need(H, 4, 2)))
    for budget in (4 * max(need.values()), max(need.values())):
        cut = application.Parentage(samples, CANDIDATES, budget=budget, selfings=True)
        cut.add_block(units, ploidy_of, flat)
        assert cut.skipped == whole.skipped and all(np.array_equal(cut.sums[c], whole.sums[c]) for c in whole.plan.progeny)
    small = application.Parentage(samples, CANDIDATES, budget=max(need.values()) - 1, selfings=True)
    small.add_block(units, ploidy_of, flat)
    big = sum(1 for u in units if need[len(u["locus"].haplotypes)] == max(need.values()))
    assert 0 < big < len(units) and all(small.skipped[c] == big and small.records[c] == len(units) - big for c in small.plan.progeny)
    host = application.Parentage(samples, CANDIDATES, budget=max(need.values()) - 1, selfings=True)
    host.add_block(units, ploidy_of, flat, NumpyBackend())
    _hold(small, host, len(units))


def test_with_selfings_off_the_device_table_is_the_table_without_them(block):
    from mchap_amd import application

    units, samples = block
    dev = application.Parentage(samples, CANDIDATES, selfings=False)
    dev.add_block(units, ploidy_of, flat)
    host = application.Parentage(samples, CANDIDATES)
    host.add_block(units, ploidy_of, flat, NumpyBackend())
    _compare(dev, host)
    assert "selfings" not in dev.text() and all(r["parent_1"] != r["parent_2"] or r["parent_1"] == "." for r in dev.table())
    on = application.Parentage(samples, CANDIDATES, selfings=True)
    on.add_block(units, ploidy_of, flat)
    for c in on.plan.progeny:                                          # the rows the two share: equal bits
        keep = [k for k, (p, q) in enumerate(on.plan.hypotheses[c]) if p != q or p == "."]
        assert np.array_equal(on.sums[c][keep], dev.sums[c])
