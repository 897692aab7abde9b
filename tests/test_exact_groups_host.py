"""Host side of `call-exact`'s grouping (application._run_exact_groups): a group larger than device_unit_budget is cut into
chunks of its members (a plain loop over the caller's units; it used to recurse on copies of them); a chunk the device batch
refuses (NotImplementedError: more than 2^62 genotypes, a workspace beyond the device) must mark the CALLER's records
FILTER=LIMIT, or those records keep invalid None without results and the record formatter raises KeyError in the middle of the
file; and cutting changes no result, each chunk padded to its own deepest unit.  No GPU: the device batch is replaced."""
from types import SimpleNamespace

import numpy as np
import pytest


class _Refused:
    def __init__(self, *a, **k):
        raise NotImplementedError("refused by the test")


class _Fake:
    """A device batch that accepts: a unit's gprob is the first value of ITS CHUNK's read tensor; the tensors' shapes are recorded."""

    shapes = None   # (a list, set by the test that reads it)

    def __init__(self, reads, K, haps, counts, prior):
        self.U, self.K, self.H = len(reads), K, haps.shape[1]
        self.tag = float(reads[0, 0, 0, 0])
        self.first = reads[:, 0, 0, 0].astype(float)
        if _Fake.shapes is not None:
            _Fake.shapes.append(reads.shape)

    def run(self, streaming=True, arrays=False):
        pass

    def mode_results(self):
        U, K, H = self.U, self.K, self.H
        return (np.zeros((U, K), np.int64), np.zeros(U), np.full(U, self.tag), np.ones(U), np.full((U, H), 1.0 / H), np.ones((U, H)))


def _units(n_records, samples, seed=0, depths=None):
    rng = np.random.default_rng(seed)
    H, M, R = 5, 4, 6
    out = []
    for i in range(n_records):
        haps = rng.integers(0, 2, size=(H, M)).astype(np.int8)
        locus = SimpleNamespace(haplotypes=haps, frequencies=np.full(H, 1.0 / H), n_alleles=[2] * M, mask_reference_allele=False,
                                stop=1000 + 100 * i + M, start=1000 + 100 * i, positions=list(1000 + 100 * i + np.arange(M)))
        reads = {}
        for j, s in enumerate(samples):
            R = R if depths is None else depths[i][j]
            reads[s] = dict(dists=rng.dirichlet(np.ones(2), size=(R, M)), counts=np.ones(R, dtype=np.int64),
                            calls=rng.integers(-1, 2, size=(R, M)).astype(np.int8), depth=np.full(M, float(R)))
        out.append(dict(rec=dict(chrom="c1", pos=1000 + 100 * i), locus=locus, invalid=None, needs_kernel=True, reads=reads))
    return out


@pytest.mark.parametrize("samples", [["S1", "S2"], ["S1", "S2", "S3"], ["S1"]], ids=["two-samples", "three-samples", "one-sample"])
@pytest.mark.parametrize("n_records", [1, 3])
def test_refused_chunks_mark_the_callers_records(monkeypatch, capsys, samples, n_records):
    from mchap_amd import application, device

    monkeypatch.setattr(device, "ExactDeviceBatch", _Refused)
    monkeypatch.setattr(application, "device_unit_budget", lambda *a, **k: 1)
    units = _units(n_records, samples)
    ploidy_of = lambda s: 4  # noqa: E731
    results = application._run_exact_groups(units, ploidy_of, lambda s: None, False, backend=None)
    assert results == {}
    assert [u["invalid"] for u in units] == ["LIMIT"] * n_records
    for ri, unit in enumerate(units):
        flt, info, fmt, cols = application._format_exact_record(unit, samples, results, ri, ploidy_of, (), None)
        assert flt == "LIMIT"
        assert info.startswith("AN=0;UAN=0;") and ";NS=0;" in info
        assert sorted(cols) == sorted(samples)
        assert all(c.split(":")[0] == "./././." for c in cols.values())
    err = capsys.readouterr().err
    assert err.count("FILTER=LIMIT") >= n_records


def test_chunks_the_device_takes_are_called(monkeypatch):
    """The same chunk path with a device batch that accepts: every (record, sample) gets its chunk's result, nothing is marked."""
    from mchap_amd import application, device

    monkeypatch.setattr(device, "ExactDeviceBatch", _Fake)
    monkeypatch.setattr(application, "device_unit_budget", lambda *a, **k: 1)
    samples = ["S1", "S2"]
    units = _units(3, samples, seed=1)
    results = application._run_exact_groups(units, lambda s: 4, lambda s: None, False, backend=None)
    assert all(u["invalid"] is None for u in units)
    assert sorted(results) == sorted((ri, s) for ri in range(3) for s in samples)
    for (ri, s), v in results.items():
        assert v["gprob"] == units[ri]["reads"][s]["dists"][0, 0, 0]  # (each unit's own chunk)


def test_chunks_give_the_results_of_the_whole_group(monkeypatch):
    """Three records by three samples of one shape, every unit of another depth, with a budget of 1, of 4 and of the whole group: the
    same results, and every chunk's read tensor is padded to the deepest unit of THAT chunk (the exact kernel sums the reads four to a
    logarithm: the padding is part of what a unit computes, so a chunk must not be padded to the group's depth)."""
    from mchap_amd import application, device

    class _PerUnit(_Fake):
        def mode_results(self):
            out = list(super().mode_results())
            out[2] = self.first   # (gprob: each unit's own first value, whatever chunk it came in)
            return tuple(out)

    monkeypatch.setattr(device, "ExactDeviceBatch", _PerUnit)
    samples = ["S1", "S2", "S3"]
    depths = [[3, 9, 4], [7, 2, 8], [5, 6, 1]]
    flat = [d for row in depths for d in row]   # (the group's members: record by record, sample by sample)
    got = {}
    for budget in (1, 4, 1 << 20):
        monkeypatch.setattr(application, "device_unit_budget", lambda *a, budget=budget, **k: budget)
        monkeypatch.setattr(_Fake, "shapes", [])
        units = _units(3, samples, seed=2, depths=depths)
        got[budget] = application._run_exact_groups(units, lambda s: 4, lambda s: None, False, backend=None)
        assert all(u["invalid"] is None for u in units)
        step = min(budget, 9)
        assert [sh[:2] for sh in _Fake.shapes] == [(len(flat[c:c + step]), max(flat[c:c + step])) for c in range(0, 9, step)]
    assert sorted(got[1]) == sorted((ri, s) for ri in range(3) for s in samples)
    for budget in (4, 1 << 20):
        assert sorted(got[budget]) == sorted(got[1])
        for key, v in got[1].items():
            assert sorted(v) == sorted(got[budget][key])
            for name in v:
                np.testing.assert_array_equal(v[name], got[budget][key][name])
