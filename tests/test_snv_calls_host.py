"""call-exact --snv-calls on the host: call_exact(..., calling=<the oracle>, snv_calls=SnvCalls(...)) on the reference's BAM / VCF
files -- the record lines unchanged, the SNV file `atomize` of those lines in every field but GQ, DS and ACP (and GP when asked),
DS the ACP the main VCF reports projected onto the SNVs, GQ a whole number where there is a call.  CPU only."""
import os
from math import comb

import numpy as np
import pytest

from mchap_amd import application, atomize
from mchap_amd.io import vcf_record

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
BAMS = ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")
SAMPLES = ["SAMPLE1", "SAMPLE2", "SAMPLE3"]
VCF = os.path.join(HERE, "mock.input.frequencies.vcf")


@pytest.fixture(scope="module")
def oracle():
    from tests.replay_call_exact import OracleBackend

    return OracleBackend()


def _bams():
    return {s: os.path.join(HERE, f) for s, f in zip(SAMPLES, BAMS)}


def _fields(line):
    f = line.split("\t")
    info = dict(kv.split("=", 1) for kv in f[7].split(";"))
    return f, info, [dict(zip(f[8].split(":"), col.split(":"))) for col in f[9:]]


def _compare(snv_lines, plain_lines, gp):
    """The SNV lines against `atomize` of the record lines: every field but GQ, DS, ACP (and GP) equal; DS and ACP within the
    rounding of the record's own ACP."""
    want, n_haps = [], []
    for line in plain_lines:
        rec = vcf_record(line.split("\t"), SAMPLES)
        block = atomize.snv_block_lines(rec, SAMPLES)
        want += block
        n_haps += [1 + len(rec["alts"])] * len(block)
    assert len(snv_lines) == len(want) >= 5
    n_gq = 0
    for got_line, want_line, H_rec in zip(snv_lines, want, n_haps):
        g, ginfo, gcols = _fields(got_line)
        w, winfo, wcols = _fields(want_line)
        assert g[:7] == w[:7] and g[8] == w[8] + (":GP" if gp else "")
        assert {k: v for k, v in ginfo.items() if k != "ACP"} == {k: v for k, v in winfo.items() if k != "ACP"}
        A = 1 + (len(g[4].split(",")) if g[4] else 0)   # the SNV's alleles
        for gc, wc in zip(gcols, wcols):
            assert {k: gc[k] for k in ("GT", "PQ", "DP")} == {k: wc[k] for k in ("GT", "PQ", "DP")}
            called = "." not in gc["GT"]
            if called:
                assert gc["GQ"] == str(int(gc["GQ"])) and 0 <= int(gc["GQ"]) <= 60
                n_gq += 1
                # the record's ACP is written to 3 decimals per haplotype: up to H of them add up in an SNV allele's count, and the
                # normalisation to the ploidy moves it by as much again; DS is itself rounded; and the oracle's caller forms its
                # posterior from float64 likelihoods, the definition here from its float32 array (1e-4 covers that)
                tol = 0.0005 * (2 * H_rec + 1) + 1e-4
                if wc["DS"] != ".":
                    assert np.allclose([float(x) for x in gc["DS"].split(",")], [float(x) for x in wc["DS"].split(",")], rtol=0, atol=tol)
            else:
                assert gc["GQ"] == "." and set(gc["DS"].split(",")) == {"."}   # (one '.' per ALT, as the reference writes NaN)
            if gp:
                K = len(gc["GT"].split("|"))
                probs = [float(x) for x in gc["GP"].split(",")] if called else []
                if called:
                    assert len(probs) == comb(A + K - 1, K) and abs(sum(probs) - 1.0) <= 0.0005 * len(probs) + 1e-9
    return n_gq


@pytest.mark.parametrize("kw", [dict(inbreeding=0.1, prior_frequencies_tag="AFP"), dict()], ids=["dirmul", "flat"])
def test_the_snv_file_of_a_run(oracle, kw):
    kw = dict(ploidy=4, report=("ACP", "SNVDP"), calling=oracle, **kw)
    plain = list(application.call_exact(VCF, _bams(), **kw))
    snv = application.SnvCalls(SAMPLES, atomize.vcf_contig_lines(VCF))
    assert list(application.call_exact(VCF, _bams(), snv_calls=snv, **kw)) == plain          # the record lines are unchanged
    assert _compare(snv.lines, plain, gp=False) >= 10
    # --report changes nothing in DS / ACP: present without the record's ACP too
    bare = dict(kw, report=())
    snv2 = application.SnvCalls(SAMPLES)
    bare_lines = list(application.call_exact(VCF, _bams(), snv_calls=snv2, **bare))
    assert bare_lines == list(application.call_exact(VCF, _bams(), **bare))
    pick = lambda ln: (_fields(ln)[1]["ACP"], [(c["GQ"], c["DS"]) for c in _fields(ln)[2]])
    assert [pick(ln) for ln in snv2.lines] == [pick(ln) for ln in snv.lines]
    # one record per block: the same SNV file
    snv3 = application.SnvCalls(SAMPLES, atomize.vcf_contig_lines(VCF))
    assert list(application.call_exact(VCF, _bams(), snv_calls=snv3, records_per_block=1, **kw)) == plain and snv3.lines == snv.lines
    # GP
    snv4 = application.SnvCalls(SAMPLES, atomize.vcf_contig_lines(VCF), report=("GP",))
    assert list(application.call_exact(VCF, _bams(), snv_calls=snv4, **kw)) == plain
    _compare(snv4.lines, plain, gp=True)
    assert [[c.rsplit(":", 1)[0] for c in ln.split("\t")[9:]] for ln in snv4.lines] == [ln.split("\t")[9:] for ln in snv.lines]
    head, head4 = snv.header(), snv4.header()
    assert [ln for ln in head4 if ln not in head] == ['##FORMAT=<ID=GP,Number=G,Type=Float,Description="Genotype posterior probabilities">']
    assert head[-1].split("\t")[9:] == SAMPLES and any(ln.startswith("##contig=") for ln in head)
    assert snv.text() == "\n".join(head + snv.lines) + "\n"


def test_the_posteriors_are_the_definition(oracle):
    """add_block's arrays are snv_posterior_unit of the oracle's likelihoods; their dosages are K times the caller's own posterior
    allele frequencies projected onto the SNVs (the caller's float64 posterior against one formed from its float32 likelihoods)."""
    _, records = application.read_vcf(VCF)
    source = application.ReadSource(_bams())
    units = application._exact_units(records, source, SAMPLES, "AFP", None, False)
    results = application._run_exact_groups(units, lambda s: 4, lambda s: 0.1, False, oracle)
    post = application.snv_posteriors_host(units, SAMPLES, lambda s: 4, lambda s: 0.1, oracle)
    assert sorted(post) == sorted(results) and len(post) >= 3
    table = application._genotype_table(4, 4)
    for (ri, s), p in post.items():
        haps = units[ri]["locus"].haplotypes
        assert p.shape[0] == haps.shape[1] and np.allclose(p.sum(axis=1), 1.0, atol=1e-12)
        for j in range(haps.shape[1]):
            for a in range(int(haps[:, j].max()) + 1):
                copies = (table[:p.shape[1]] == a).sum(axis=1)
                want = 4 * results[(ri, s)]["freqs"][haps[:, j] == a].sum()
                assert abs(p[j] @ copies - want) <= 1e-4, (ri, s, j, a)


def test_null_calls_and_a_single_haplotype(oracle):
    """An invalid record (every prior frequency 0) has null calls: GQ and DS are '.'.  A record with one haplotype and an SNVPOS
    needs no kernel: probability 1."""
    snv = application.SnvCalls(["A", "B"])
    unit = dict(invalid=None, needs_kernel=False)
    lines = ["C1\t10\tr1\tACGT\t.\t.\tPASS\tSNVPOS=2\tGT:GQ:SQ\t0/0:60:60\t0/0/0:60:60",
             "C1\t30\tr2\tACGT\tAGGT\t.\tAF0\tSNVPOS=2\tGT:GQ:SQ\t./.:.:.\t././.:.:."]
    post = snv.add_block([unit, dict(invalid="AF0", needs_kernel=False)], lines, lambda s: 2, lambda s: None, oracle)
    assert post == {}
    got = [ln.split("\t") for ln in snv.lines]
    assert got[0][:5] == ["C1", "11", "r1_SNV1", "C", ""] and got[0][7] == "AC=;ACP=5;DP=.;PS=10"
    assert got[0][9:] == ["0|0:60:60:.:", "0|0|0:60:60:.:"]
    assert got[1][:5] == ["C1", "31", "r2_SNV1", "C", "G"] and got[1][7] == "AC=0;ACP=.,.;DP=.;PS=30"
    assert got[1][9:] == [".|.:.:.:.:.", ".|.|.:.:.:.:."]
    with pytest.raises(ValueError, match="GP"):
        application.SnvCalls(["A"], report=("GL",))
    with pytest.raises(ValueError, match="single process"):
        list(application.call_exact(VCF, _bams(), calling=oracle, shard=(0, 2), snv_calls=application.SnvCalls(SAMPLES)))
    with pytest.raises(ValueError, match="samples"):
        list(application.call_exact(VCF, _bams(), calling=oracle, snv_calls=application.SnvCalls(["A"])))
