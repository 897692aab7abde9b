"""call-exact --allele-depths on the host: call_exact(..., calling=<the oracle>, allele_depths=AlleleDepths(...)) on the reference's
BAM / VCF files -- the record lines unchanged, the file's lines those lines with ADP added to INFO, FORMAT and every sample, a
sample's ADP summing to its read weight, INFO the samples' sum, the null rules, one record per block.  CPU only."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from mchap_amd import application

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
BAMS = ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")
SAMPLES = ["SAMPLE1", "SAMPLE2", "SAMPLE3"]
VCF = os.path.join(HERE, "mock.input.frequencies.vcf")
HEADER = ["##fileformat=VCFv4.3", '##INFO=<ID=AN,Number=1,Type=Integer,Description="x">', '##INFO=<ID=AC,Number=A,Type=Integer,Description="x">',
          '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(SAMPLES)]


@pytest.fixture(scope="module")
def oracle():
    from tests.replay_call_exact import OracleBackend

    return OracleBackend()


def _bams():
    return {s: os.path.join(HERE, f) for s, f in zip(SAMPLES, BAMS)}


def _numbers(text):
    return [np.nan if x == "." else float(x) for x in text.split(",")]


def _split(line):
    """(the line without ADP, INFO ADP, [sample ADP])."""
    f = line.split("\t")
    info = f[7].split(";")
    assert info[-1].startswith("ADP=") and f[8].endswith(":ADP")
    cols = [c.rsplit(":", 1) for c in f[9:]]
    plain = "\t".join(f[:7] + [";".join(info[:-1]), f[8][:-4]] + [c[0] for c in cols])
    return plain, _numbers(info[-1][4:]), [_numbers(c[1]) for c in cols]


def _units(tag):
    _, records = application.read_vcf(VCF)
    return application._exact_units(records, application.ReadSource(_bams()), SAMPLES, tag, None, False)


@pytest.mark.parametrize("kw", [dict(inbreeding=0.1, prior_frequencies_tag="AFP"), dict()], ids=["dirmul", "flat"])
def test_the_file_of_a_run(oracle, kw):
    kw = dict(ploidy=4, report=("ACP",), calling=oracle, **kw)
    plain = list(application.call_exact(VCF, _bams(), **kw))
    depths = application.AlleleDepths(SAMPLES, HEADER)
    assert list(application.call_exact(VCF, _bams(), allele_depths=depths, **kw)) == plain      # the record lines are unchanged
    assert len(depths.lines) == len(plain) >= 3
    units = _units(kw.get("prior_frequencies_tag"))
    n_numbers = 0
    for line, want, unit in zip(depths.lines, plain, units):
        got, info, cols = _split(line)
        assert got == want
        H = len(unit["locus"].haplotypes)
        assert len(info) == H and all(len(c) == H for c in cols)
        total = np.zeros(H)
        for s, c in zip(SAMPLES, cols):
            if unit["invalid"] is not None:
                assert np.all(np.isnan(c))
                continue
            n_numbers += 1
            weight = float(np.sum(unit["reads"][s]["counts"]))
            assert abs(np.sum(c) - weight) <= 0.0005 * H + 1e-9 and min(c) >= 0.0     # written to 3 decimals
            total += c
        if unit["invalid"] is not None:
            assert np.all(np.isnan(info))
        else:
            np.testing.assert_allclose(info, total, rtol=0, atol=0.0005 * (len(SAMPLES) + 1))
    assert n_numbers >= 6
    # one record per block: the same file
    each = application.AlleleDepths(SAMPLES, HEADER)
    assert list(application.call_exact(VCF, _bams(), allele_depths=each, records_per_block=1, **kw)) == plain and each.lines == depths.lines
    # the header: the run's own with the two declarations after the last INFO and the last FORMAT line
    head = depths.header()
    assert [ln for ln in head if ln not in HEADER] == [
        '##INFO=<ID=ADP,Number=R,Type=Float,Description="Posterior expected read depth of each allele">',
        '##FORMAT=<ID=ADP,Number=R,Type=Float,Description="Posterior expected read depth of each allele">']
    assert [ln for ln in head if ln in HEADER] == HEADER and head.index(head[3]) == 3 and head[3].startswith("##INFO=<ID=ADP") and \
        head[5].startswith("##FORMAT=<ID=ADP") and head[-1] == HEADER[-1]
    assert depths.text() == "\n".join(head + depths.lines) + "\n"


def test_the_depths_are_the_definition(oracle):
    """add_block's arrays are allele_support_unit of the oracle's likelihoods; together with the frequency estimate the estimated
    prior is the one used."""
    units = _units("AFP")
    ploidy_of, inbreeding_of = (lambda s: 4), (lambda s: 0.1)
    got = application.AlleleDepths(SAMPLES).add_block(units, ["\t".join(["c", "1", ".", "A", ".", ".", "PASS", "AN=0", "GT"] + ["."] * 3)] * len(units),
                                                     ploidy_of, inbreeding_of, oracle)
    n = 0
    for (ri, s), depth in got.items():
        unit = units[ri]
        sr, locus = unit["reads"][s], unit["locus"]
        if len(sr["counts"]) == 0:
            assert np.all(depth == 0.0)
            continue
        llk = np.asarray(oracle.genotype_likelihoods(sr["dists"], 4, locus.haplotypes, read_counts=sr["counts"]), dtype=np.float64)
        want, post = application.allele_support_unit(sr["dists"], sr["counts"], locus.haplotypes, llk, 4, 0.1, locus.frequencies)
        assert np.array_equal(depth, want)
        np.testing.assert_allclose(post[np.asarray(sr["counts"]) > 0].sum(axis=1), 1.0, rtol=0, atol=1e-9)
        n += 1
    assert n >= 3
    before = [u["locus"].frequencies.copy() for u in units]
    application.estimate_prior_frequencies(units, SAMPLES, ploidy_of, inbreeding_of, 3, backend=oracle)
    assert any(not np.array_equal(a, u["locus"].frequencies) for a, u in zip(before, units))
    after = application.allele_support_host(units, SAMPLES, ploidy_of, inbreeding_of, oracle)
    assert any(not np.array_equal(after[key], got[key]) for key in got)


class _NoFiniteGenotype:
    def __init__(self, inner):
        self.inner = inner

    def genotype_likelihoods(self, *a, **kw):
        return np.full(len(self.inner.genotype_likelihoods(*a, **kw)), -np.inf)


def test_the_null_rules(oracle, monkeypatch):
    line = "\t".join(["c", "1", ".", "A", "C,G", ".", "PASS", "AN=0", "GT"] + ["0/0/0/0"] * 3)
    units = [u for u in _units("AFP") if u["needs_kernel"]][:1]
    H = len(units[0]["locus"].haplotypes)
    null = ",".join(["."] * H)
    ploidy_of, inbreeding_of = (lambda s: 4), (lambda s: 0.1)

    def written(units, backend=oracle):
        depths = application.AlleleDepths(SAMPLES)
        depths.add_block(units, [line] * len(units), ploidy_of, inbreeding_of, backend)
        return [_split(ln) for ln in depths.lines], depths.lines

    (plain, info, cols), = written(units)[0]
    assert plain == line and not np.any(np.isnan(info)) and not np.any(np.isnan(cols))
    # an invalid record, FILTER=LIMIT among them: every sample and INFO null -- one '.' per allele, as a null ACP
    for invalid in ("AF0", "LIMIT"):
        (_, info, cols), = written([dict(units[0], invalid=invalid)])[0]
        assert np.all(np.isnan(info)) and np.all(np.isnan(cols))
        assert written([dict(units[0], invalid=invalid)])[1][0].split("\t")[7].endswith(";ADP=" + null)
    # no finite genotype
    (_, info, cols), = written(units, _NoFiniteGenotype(oracle))[0]
    assert np.all(np.isnan(info)) and np.all(np.isnan(cols))
    # a refused shape
    monkeypatch.setattr(application, "_support_evaluable", lambda unit, K: False)
    (_, info, cols), = written(units)[0]
    assert np.all(np.isnan(info)) and np.all(np.isnan(cols))
    monkeypatch.undo()
    # a sample without reads: zeros; INFO is the sum of the samples that have a number
    M, A = units[0]["reads"][SAMPLES[0]]["dists"].shape[1:]
    empty = dict(units[0]["reads"][SAMPLES[0]], counts=np.zeros(0, dtype=np.int64), dists=np.zeros((0, M, A)))
    (_, info, cols), = written([dict(units[0], reads=dict(units[0]["reads"], **{SAMPLES[0]: empty}))])[0]
    assert cols[0] == [0.0] * H and abs(sum(info) - sum(cols[1]) - sum(cols[2])) <= 0.002
    # a single haplotype needs no kernel: its one allele gets the sample's read weight
    one = dict(invalid=None, needs_kernel=False, locus=SimpleNamespace(haplotypes=np.zeros((1, 2), dtype=np.int8)),
               reads={s: dict(counts=np.array([2, 1, 4]) * (i + 1)) for i, s in enumerate(SAMPLES)})
    (_, info, cols), = written([one])[0]
    assert cols == [[7.0], [14.0], [21.0]] and info == [42.0]
    (_, info, cols), = written([dict(one, invalid="NOA")])[0]
    assert np.all(np.isnan(info)) and np.all(np.isnan(cols))


def test_errors(oracle):
    with pytest.raises(ValueError, match="single process"):
        list(application.call_exact(VCF, _bams(), calling=oracle, shard=(0, 2), allele_depths=application.AlleleDepths(SAMPLES)))
    with pytest.raises(ValueError, match="samples"):
        list(application.call_exact(VCF, _bams(), calling=oracle, allele_depths=application.AlleleDepths(["A"])))
