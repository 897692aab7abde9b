"""The trace-summary kernels -- trace_posterior_kernel<8|32>, trace_incongruence_kernel<8|32> (csrc/posterior_kernel.hpp) -- driven
through the C entry points with built traces (tests/trace_summary_cases.py: each case named for the branch it reaches, in every form
it applies to -- one word per haplotype, two words, the calling form) against the plain definition of
tests/trace_summary_reference.py, which tests/test_trace_summary_reference.py anchors on the host classes.  Distinct states and their
order, counts, post_n, mode_index / mode_words / mode_count, GPM and MCI are compared exactly; SPM with the exact Fraction, within
2 t 2^-53 for a mode support of t genotypes (one rounding per term count / N and one per addition, each of a value at most 1).
Every launch is a batch call and a listed call, each made twice with bit-equal outputs."""
import pytest

from tests import trace_summary_cases as cases
from tests.fuzz_trace_summary import batch_cap, check_launch, max_cap, run, run_launch

pytestmark = pytest.mark.gpu

WORST = {}   # form kind -> the worst SPM deviation as a fraction of its bound, over what has run


@pytest.fixture(scope="module")
def L():
    from mchap_amd import _lib

    return _lib.lib()


def _note(launch, worst):
    WORST[launch.form.kind] = max(WORST.get(launch.form.kind, 0.0), worst)


def test_a_batch_launch_keeps_512_states_in_every_form(L):
    """min(512, mchap_trace_posterior_max_states_wph) is 512 for every ploidy_max the cases use: `full-table` is built for that."""
    for launch in cases.all_launches():
        assert batch_cap(L, launch) == cases.BATCH_CAP == 512
        assert max_cap(L, launch.ploidy_max, launch.form.W) >= cases.LISTED_CAP


@pytest.mark.parametrize("name", list(cases.CASES))
def test_built_traces_against_the_definition(L, name):
    launches = cases.launches(name)
    assert launches
    codes = {}
    for launch in launches:
        worst, seen = check_launch(L, launch, run_launch(L, launch))
        _note(launch, worst)
        codes.setdefault(launch.form.id, set()).update(seen)
        print("%s %s: SPM within %.3g of its bound, codes %s" % (launch.name, launch.form.id, worst, sorted(seen)))
    if name == "mci-codes":   # per form, the kernels produced every code
        assert len(codes) == len(cases.FORMS) and all(v == {0, 1, 2} for v in codes.values()), codes
    if name in ("high-word-only", "low-word-only"):
        assert all(v == {0, 1, 2} for v in codes.values()), codes


def test_the_overflow_and_the_refusal_were_reached(L):
    """`full-table` and `ragged-ploidy` as the caller sees them: the sign of post_n, mci = -1, INT32_MIN -- beside the comparison
    above, which takes the same branches by the definition's counts."""
    import numpy as np

    for launch in cases.launches("full-table"):
        out = run_launch(L, launch)
        batch = launch.name.endswith("batch")
        got = out["batch" if batch else "listed"]
        cap = cases.BATCH_CAP if batch else cases.LISTED_CAP
        rows = {u: i for i, u in enumerate(launch.unit_list)} if not batch else {u: u for u in range(4)}
        assert got["n"][0] == cap and got["n"][3] == cap and got["n"][1] < 0 and got["n"][2] < 0
        assert -int(got["n"][1]) >= cap + 1 and -int(got["n"][2]) >= cap + 1
        assert got["mci"][2] == -1 and (got["mci"][[0, 1, 3]] >= 0).all()
        assert got["counts"][rows[0]].sum() + got["counts"][rows[3]].sum() > 0
    for launch in cases.launches("ragged-ploidy"):
        out = run_launch(L, launch)
        n = out["batch"]["n"]
        if launch.name.endswith("one-above"):
            big = int(np.argmax([K for K, _ in launch.units]))
            assert n[big] == -2 ** 31 and out["batch"]["mci"][big] == -1 and (np.delete(n, big) > 0).all()
        else:
            assert (n > 0).all()
            KW = launch.ploidy_max * launch.form.W
            for u, (K, _) in enumerate(launch.units):   # rows are zero beyond the unit's own words
                assert not out["batch"]["words"][u, :, K * launch.form.W:KW].any() and not out["batch"]["mw"][u, K * launch.form.W:].any()
                assert out["batch"]["words"][u, 0, :K * launch.form.W].any()


def test_truncated_rows_and_the_mode_beyond_them(L):
    for launch in cases.launches("truncated"):
        got = run_launch(L, launch)["batch"]
        for u in range(len(launch.units)):
            assert got["n"][u] == 9 and got["mode"][u] >= 4 and got["counts"][u].tolist() == [10] * 4 and got["mc"][u] == 6
            assert got["mw"][u].any()


def test_listed_subset_leaves_the_other_units_alone(L):
    for launch in cases.launches("listed-subset"):
        assert launch.unit_list == [3, 1] and len(launch.units) == 5
        out = run_launch(L, launch)
        b, l = out["batch"], out["listed"]
        assert l["counts"].shape[0] == 2
        assert l["counts"][0, :5].tolist() == b["counts"][3, :5].tolist() and l["counts"][1, :3].tolist() == b["counts"][1, :3].tolist()
        assert b["n"].tolist() == [2, 3, 4, 5, 6] == l["n"].tolist()


FUZZ_SEEDS = (91, 92, 93)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_random_walks_against_the_definition(seed):
    units, worst, seen = run(9, seed)
    print("seed %d: %d units, SPM within %.3g of its bound, codes %s" % (seed, units, worst, sorted(seen)))
    assert units >= 36


def test_the_fuzz_seeds_mix_the_forms():
    """All three forms, ploidies below ploidy_max, and tables smaller than the distinct states are among what the seeds draw."""
    from tests.fuzz_trace_summary import drawn
    from tests.trace_summary_reference import distinct_count

    kinds, ragged, over, shared = set(), 0, 0, [0, 0]
    for seed in FUZZ_SEEDS:
        for launch in drawn(9, seed):
            kinds.add(launch.form.kind)
            ragged += any(K < launch.ploidy_max for K, _ in launch.units)
            over += any(distinct_count(launch.burnt(u)) > launch.cap for u in launch.unit_list)
            if launch.form.W == 2:
                for u in range(len(launch.units)):
                    haps = sorted({h for c in launch.burnt(u) for s in c for h in s})
                    for i, a in enumerate(haps):
                        for b_ in haps[:i]:
                            shared[0] += (a >> 64 == b_ >> 64) != (a & (2 ** 64 - 1) == b_ & (2 ** 64 - 1))
                            shared[1] += 1
    print("forms %s, %d ragged launches, %d with a table too small, %d of %d pairs of haplotypes share one word" % (
        sorted(kinds), ragged, over, shared[0], shared[1]))
    assert kinds == {"w1", "w2", "call"} and ragged >= 3 and over >= 3
    assert 0.3 <= shared[0] / shared[1] <= 0.7


def test_report_the_worst_spm_deviation():
    """Printed for the record: per form, the worst SPM deviation over the built cases as a fraction of 2 t 2^-53."""
    for kind in sorted(WORST):
        print("SPM, form %s: worst deviation %.3g of its bound" % (kind, WORST[kind]))
        assert WORST[kind] <= 1.0
