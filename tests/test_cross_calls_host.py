"""call-exact --cross-calls on the host: application.CrossCalls over the units of a synthetic bi-parental block
(application.MatrixSource; tests/cross_reference.py biparental_block) with a float64 numpy likelihood backend -- the three fields
of every sample, the default progeny, the sign of the log Bayes factor for progeny of the cross and for an unrelated sample, the
null rules, the frequency estimate's prior, the header, the checks of the cross.  CPU only."""
from types import SimpleNamespace

import numpy as np
import pytest

from mchap_amd import application
from mchap_amd.io import vcfstr
from tests import cross_reference as ref

PLOIDY = {"D0": 2}
HEADER = ["##fileformat=VCFv4.3", '##INFO=<ID=AN,Number=1,Type=Integer,Description="x">',
          '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', '##FORMAT=<ID=GPM,Number=1,Type=Float,Description="x">']


def ploidy_of(s):
    return PLOIDY.get(s, 4)


@pytest.fixture(scope="module")
def block():
    records, samples, matrices, truth = ref.biparental_block(depth=200, extra=PLOIDY)
    units = application._exact_units(records, application.MatrixSource(samples, matrices), samples, None, None, False)
    return units, samples, truth


def _lines(units, samples):
    return ["\t".join(["chr1", str(u["rec"]["pos"]) if "rec" in u else "1", ".", "A", ".", ".", "PASS", "AN=0", "GT:GPM"] + ["0/0:1"] * len(samples))
            for u in units]


def _written(units, samples, inbreeding_of=lambda s: None, backend=None, **kw):
    calls = application.CrossCalls(samples, ("P", "Q"), header_lines=HEADER + ["#CHROM\t" + "\t".join(samples)], **kw)
    got = calls.add_block(units, _lines(units, samples), ploidy_of, inbreeding_of, backend or ref.NumpyBackend())
    fields = []
    for line, plain in zip(calls.lines, _lines(units, samples)):
        f, p = line.split("\t"), plain.split("\t")
        assert f[:8] == p[:8] and f[8] == p[8] + ":CGT:CGPM:CLBF" and [c.rsplit(":", 3)[0] for c in f[9:]] == p[9:]
        fields.append({s: c.rsplit(":", 3)[1:] for s, c in zip(samples, f[9:])})
    return calls, got, fields


@pytest.mark.parametrize("inbreeding", [None, 0.1], ids=["flat", "dirmul"])
def test_the_fields_of_a_block(block, inbreeding):
    units, samples, truth = block
    calls, got, fields = _written(units, samples, lambda s: inbreeding)
    assert calls.cross.resolve(samples, ploidy_of)[2] == ["C0", "C1", "C2", "U0"]       # every other sample of ploidy 2 + 2
    host = application.cross_calls_host(units, samples, ploidy_of, lambda s: inbreeding, calls.cross, ref.NumpyBackend())
    assert got == host and set(got) == {(ri, s) for ri in range(len(units)) for s in ("C0", "C1", "C2", "U0")}
    for ri, row in enumerate(fields):
        for s in ("P", "Q", "D0"):
            assert row[s] == [".", ".", "."]
        for s in ("C0", "C1", "C2", "U0"):
            cgt, cgpm, clbf = row[s]
            genotype, prob, lbf = got[(ri, s)]
            assert cgt == "/".join(str(a) for a in genotype) and len(genotype) == 4 and list(genotype) == sorted(genotype)
            assert cgpm == vcfstr(prob)
            assert clbf == "%.3f" % lbf and 0.0 <= float(cgpm) <= 1.0
            # deep reads: the call is the drawn genotype, and the cross explains a progeny better than the population does --
            # an unrelated sample (of haplotypes the parents do not carry) far worse
            assert genotype == truth[(ri, s)]
            if s == "U0":
                assert lbf < -5.0
            else:
                assert lbf > 0.5
    # one record per call: the same lines
    each = application.CrossCalls(samples, ("P", "Q"))
    for u, line in zip(units, _lines(units, samples)):
        each.add_block([u], [line], ploidy_of, lambda s: inbreeding, ref.NumpyBackend())
    assert each.lines == calls.lines


def test_a_call_is_the_definition_under_the_records_frequencies(block):
    """The frequency estimate leaves its result in locus.frequencies (tests/test_cross_calls_cli.py runs the two together): those are
    the ones the parents' priors, the gamete error's multinomial and the progeny's calling prior use."""
    units, samples, _ = block
    units = [dict(u, locus=SimpleNamespace(**vars(u["locus"]))) for u in units]
    inbreeding_of = lambda s: 0.2  # noqa: E731
    backend = ref.NumpyBackend()
    cross = application.Cross(("P", "Q"), ["C1"], (0.01, 0.2))
    before = application.cross_calls_host(units, samples, ploidy_of, inbreeding_of, cross, backend)
    rng = np.random.default_rng(3)
    for u in units:
        u["locus"].frequencies = rng.dirichlet(np.full(len(u["locus"].haplotypes), 2.0))
    after = application.cross_calls_host(units, samples, ploidy_of, inbreeding_of, cross, backend)
    assert set(after) == {(ri, "C1") for ri in range(len(units))}
    assert any(before[k][1:] != after[k][1:] for k in after)
    for (ri, s), (genotype, prob, lbf) in after.items():
        locus, reads = units[ri]["locus"], units[ri]["reads"]
        H = len(locus.haplotypes)
        assert not np.allclose(locus.frequencies, 1.0 / H)
        llk = {x: backend.genotype_likelihoods(reads[x]["dists"], 4, locus.haplotypes, read_counts=reads[x]["counts"]) for x in ("P", "Q", s)}
        want = application.cross_prior_unit(llk["P"], 4, 0.2, llk["Q"], 4, 0.2, H, locus.frequencies, (0.01, 0.2), llk[s])
        norm = application._unit_posterior(llk[s], H, 4, 0.2, locus.frequencies)[1]
        assert genotype == tuple(application._genotype_table(H, 4)[want["mode"]]) and prob == want["mode_prob"] and lbf == want["log_z"] - norm


class _Dead:
    """The backend with -inf likelihoods for the read tensors listed (by identity), or for all."""

    def __init__(self, dead=None):
        self.inner, self.dead = ref.NumpyBackend(), dead

    def genotype_likelihoods(self, dists, *a, **kw):
        llk = self.inner.genotype_likelihoods(dists, *a, **kw)
        return np.full(len(llk), -np.inf) if self.dead is None or any(dists is d for d in self.dead) else llk


def test_the_null_rules(block, monkeypatch):
    units, samples, _ = block
    units = units[:1]
    null = [".", ".", "."]
    progeny = ("C0", "C1", "C2", "U0")
    assert all(_written(units, samples)[2][0][s] != null for s in progeny)
    # an invalid record, FILTER=LIMIT among them
    for invalid in ("AF0", "LIMIT"):
        assert all(v == null for v in _written([dict(units[0], invalid=invalid)], samples)[2][0].values())
    # a shape the library refuses
    monkeypatch.setattr(application, "_support_evaluable", lambda unit, K: False)
    assert all(v == null for v in _written(units, samples)[2][0].values())
    monkeypatch.undo()
    # a parent without a finite genotype: every progeny null; a progeny without: that one alone
    reads = units[0]["reads"]
    assert all(v == null for v in _written(units, samples, backend=_Dead([reads["Q"]["dists"]]))[2][0].values())
    row = _written(units, samples, backend=_Dead([reads["C1"]["dists"]]))[2][0]
    assert row["C1"] == null and all(row[s] != null for s in ("C0", "C2", "U0"))
    # a parent without reads is called from its prior alone, and the progeny still have calls
    M, A = reads["P"]["dists"].shape[1:]
    empty = dict(reads["P"], counts=np.zeros(0, dtype=np.int64), dists=np.zeros((0, M, A)))
    row = _written([dict(units[0], reads=dict(reads, P=empty))], samples)[2][0]
    assert all(row[s] != null for s in progeny)
    # a single haplotype needs no kernel: one genotype under either prior
    one = dict(invalid=None, needs_kernel=False, locus=SimpleNamespace(haplotypes=np.zeros((1, 2), dtype=np.int8)), reads={s: {} for s in samples})
    row = _written([one], samples)[2][0]
    assert all(row[s] == ["0/0/0/0", "1", "0.000"] for s in progeny) and all(row[s] == null for s in ("P", "Q", "D0"))
    assert all(v == null for v in _written([dict(one, invalid="NOA")], samples)[2][0].values())


def test_the_header_and_the_checks_of_the_cross(block):
    units, samples, _ = block
    calls = _written(units[:1], samples, progeny=["C0"], gamete_error=(0.0, 0.5))[0]
    head = calls.header()
    added = [ln for ln in head if ln not in calls.header_lines]
    assert [ln.split(",")[0] for ln in added] == ["##FORMAT=<ID=CGT", "##FORMAT=<ID=CGPM", "##FORMAT=<ID=CLBF"]
    assert ["Type=String" in added[0], "Type=Float" in added[1], "Type=Float" in added[2]] == [True] * 3 and "P and Q" in added[0]
    assert [ln for ln in head if ln in calls.header_lines] == calls.header_lines and head[4:7] == added and head[-1].startswith("#CHROM")
    assert calls.text() == "\n".join(head + calls.lines) + "\n" and calls.cross.gamete_error == (0.0, 0.5)
    for kw, message in ((dict(parents=("P", "X")), "not a sample"), (dict(parents=("P", "P")), "one sample"),
                        (dict(parents=("P", "D0")), "progeny 'C0' has ploidy 4"), (dict(parents=("P", "Q"), progeny=["D0"]), "ploidy 2"),
                        (dict(parents=("P", "Q"), progeny=["P"]), "a parent and a progeny"), (dict(parents=("P", "Q"), progeny=["nobody"]), "not a sample")):
        kw = dict(dict(progeny=["C0"]), **kw)
        with pytest.raises(ValueError, match=message):
            application.Cross(**kw).resolve(samples, ploidy_of)
    with pytest.raises(ValueError, match="even ploidy"):
        application.Cross(("P", "Q")).resolve(samples, lambda s: 3)
    for bad in (1.5, -0.1, float("nan"), (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError, match="gamete error"):
            application.Cross(("P", "Q"), gamete_error=bad)
    with pytest.raises(ValueError, match="two parents"):
        application.Cross(("P",))
