"""call-exact --model-evidence on the command line, the exact caller replaced by the oracle: the parser's defaults, every error,
the table file, and the VCF -- header included -- byte for byte what the run writes without the flags.  CPU only."""
import io as _io
import os
from types import SimpleNamespace

import numpy as np
import pytest

from mchap_amd import application, cli

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
BAMS = ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")
SAMPLES = ["SAMPLE1", "SAMPLE2", "SAMPLE3"]
PRIOR = ["--use-dirmul-prior", "0.1", "AFP"]
HEADER = "SAMPLE\tPLOIDY\tINBREEDING\tRECORDS\tSKIPPED\tLOG_EVIDENCE\tDELTA\tCONFIGURED"


@pytest.fixture(scope="module")
def oracle():
    from tests.replay_call_exact import OracleBackend

    return OracleBackend()


def _cli(monkeypatch, oracle, extra):
    """`call-exact` of the golden job with prior frequencies through cli.run -> the text written to stdout."""
    real = application.call_exact
    monkeypatch.setattr(application, "call_exact", lambda *a, **kw: real(*a, calling=oracle, **kw))
    argv = ["mchap_amd", "call-exact", "--haplotypes", os.path.join(HERE, "mock.input.frequencies.vcf"), "--ploidy", "4", "--bam"] + \
        [os.path.join(HERE, f) for f in BAMS] + ["--report", "AFPRIOR", "AFP"] + extra
    out = _io.StringIO()
    try:
        cli.run(argv, out)
    finally:
        monkeypatch.undo()
    return out.getvalue()


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("# ") and lines[1] == HEADER
    return lines[0], [ln.split("\t") for ln in lines[2:-1]]


def test_parser_defaults_and_help():
    args = cli.build_parser("call-exact").parse_args([])
    assert args.model_evidence == [None] and args.evidence_ploidy is None and args.evidence_inbreeding is None
    args = cli.build_parser("call-exact").parse_args(["--model-evidence", "t.tsv", "--evidence-ploidy", "2", "4", "6",
                                                      "--evidence-inbreeding", "0", "0.25"])
    assert args.model_evidence == ["t.tsv"] and args.evidence_ploidy == [2, 4, 6] and args.evidence_inbreeding == [0.0, 0.25]
    helps = {a.option_strings[0]: a.help for a in cli.build_parser("call-exact")._actions if a.option_strings}
    for flag in cli.EVIDENCE_FLAGS:
        assert helps[flag].startswith("(not a reference flag)")
        assert flag not in cli.build_parser("call").format_help() and flag not in cli.build_parser("assemble").format_help()


def test_the_vcf_is_unchanged_and_the_table_is_written(monkeypatch, oracle, tmp_path):
    plain = _cli(monkeypatch, oracle, PRIOR)
    path = str(tmp_path / "evidence.tsv")
    flags = ["--model-evidence", path, "--evidence-ploidy", "2", "4", "--evidence-inbreeding", "0.1", "0.5", "0"]
    assert _cli(monkeypatch, oracle, PRIOR + flags) == plain           # header (its command line too) and records, byte for byte
    first, rows = _table(path)
    n_records = len([ln for ln in plain.splitlines() if not ln.startswith("#")])
    assert first == "# mchap_amd call-exact model evidence; frequencies: tag AFP; records: %d" % n_records
    assert [r[0] for r in rows] == [s for s in SAMPLES for _ in range(6)]
    assert [(r[1], r[2]) for r in rows[:6]] == [("2", "0.1"), ("2", "0.5"), ("2", "0"), ("4", "0.1"), ("4", "0.5"), ("4", "0")]
    assert [r[7] for r in rows[:6]] == ["0", "0", "0", "1", "0", "0"]
    for s in SAMPLES:
        mine = [r for r in rows if r[0] == s]
        assert len({(r[3], r[4]) for r in mine}) == 1 and int(mine[0][3]) >= 1 and mine[0][4] == "0"
        assert max(float(r[6]) for r in mine) == 0.0 and sum(r[6] == "0.000000" for r in mine) >= 1
        for r in mine:
            assert r[5] == "%.6f" % float(r[5]) and float(r[5]) < 0.0
            assert abs(float(r[6]) - (float(r[5]) - max(float(q[5]) for q in mine))) < 1.1e-6
    # the flags in other places of the command line, and "=" forms: still the same VCF
    assert _cli(monkeypatch, oracle, ["--model-evidence=" + str(tmp_path / "other.tsv")] + PRIOR + ["--evidence-ploidy", "2"]) == plain
    # abbreviated flags, as argparse takes them: taken out of the header's command line too
    short = ["--model-ev", str(tmp_path / "short.tsv"), "--evidence-p", "2", "4", "--evidence-i", "0.1", "0.5", "0"]
    assert _cli(monkeypatch, oracle, PRIOR + short) == plain and open(tmp_path / "short.tsv").read() == open(path).read()
    # the blocks of records do not change the table: one record per block
    again = str(tmp_path / "again.tsv")
    real = application.call_exact
    monkeypatch.setattr(application, "call_exact", lambda *a, **kw: real(*a, calling=oracle, records_per_block=1, **kw))
    out = _io.StringIO()
    cli.run(["mchap_amd", "call-exact", "--haplotypes", os.path.join(HERE, "mock.input.frequencies.vcf"), "--ploidy", "4", "--bam"] +
            [os.path.join(HERE, f) for f in BAMS] + ["--report", "AFPRIOR", "AFP"] + PRIOR +
            ["--model-evidence", again] + flags[2:], out)
    monkeypatch.undo()
    assert out.getvalue() == plain and open(again).read() == open(path).read()


def test_the_defaults_the_flat_prior_and_the_estimate(monkeypatch, oracle, tmp_path):
    path = str(tmp_path / "e.tsv")
    # defaults: the sample's own pair
    _cli(monkeypatch, oracle, PRIOR + ["--model-evidence", path])
    first, rows = _table(path)
    assert [(r[0], r[1], r[2], r[6], r[7]) for r in rows] == [(s, "4", "0.1", "0.000000", "1") for s in SAMPLES]
    own = rows
    # without a Dirichlet-multinomial prior: one flat-prior row per ploidy
    plain = _cli(monkeypatch, oracle, [])
    assert _cli(monkeypatch, oracle, ["--model-evidence", path, "--evidence-ploidy", "4", "2"]) == plain
    first, rows = _table(path)
    assert first.split("; ")[1] == "frequencies: flat"
    assert [(r[0], r[1], r[2], r[7]) for r in rows] == [(s, K, ".", c) for s in SAMPLES for K, c in (("4", "1"), ("2", "0"))]
    # a prior without a tag: flat frequencies
    args = SimpleNamespace(model_evidence=[path], evidence_ploidy=None, evidence_inbreeding=None)
    assert cli.model_evidence_settings(args, SAMPLES, 0.1, None, None, 1).frequency_source == "flat"
    assert cli.model_evidence_settings(args, SAMPLES, 0.1, "AFP", None, 1).frequency_source == "tag AFP"
    # after the estimate: the evidence is conditioned on the estimated frequencies
    with_estimate = _cli(monkeypatch, oracle, PRIOR + ["--estimate-prior-frequencies", "3"])
    assert _cli(monkeypatch, oracle, PRIOR + ["--estimate-prior-frequencies", "3", "--model-evidence", path]) == with_estimate
    first, rows = _table(path)
    assert first.split("; ")[1] == "frequencies: estimated"
    assert [r[:5] for r in rows] == [r[:5] for r in own] and [r[5] for r in rows] != [r[5] for r in own]
    # --filter-input-haplotypes: the records that are called take part
    flt = ["--filter-input-haplotypes", "AFP>=0.1"]
    assert _cli(monkeypatch, oracle, PRIOR + flt + ["--model-evidence", path]) == _cli(monkeypatch, oracle, PRIOR + flt)
    assert len(_table(path)[1]) == 3


@pytest.mark.parametrize("extra, message", [
    (["--evidence-ploidy", "2"], "--evidence-ploidy needs --model-evidence"),
    (PRIOR + ["--evidence-inbreeding", "0.1"], "--evidence-inbreeding needs --model-evidence"),
    (["--model-evidence", "x.tsv", "--evidence-inbreeding", "0.1"], "--evidence-inbreeding needs --use-dirmul-prior"),
    (["--model-evidence", "x.tsv", "--evidence-ploidy", "0"], "1..15"),
    (["--model-evidence", "x.tsv", "--evidence-ploidy", "4", "16"], "1..15"),
    (PRIOR + ["--model-evidence", "x.tsv", "--evidence-inbreeding", "0.1", "1.0"], r"\[0, 1\)"),
    (PRIOR + ["--model-evidence", "x.tsv", "--evidence-inbreeding", "-0.01"], r"\[0, 1\)"),
    (PRIOR + ["--model-evidence", "x.tsv", "--evidence-inbreeding", "nan"], r"\[0, 1\)"),
    (PRIOR + ["--model-evidence", "x.tsv", "--evidence-inbreeding", "inf"], r"\[0, 1\)"),
])
def test_errors(monkeypatch, oracle, tmp_path, extra, message):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=message):
        _cli(monkeypatch, oracle, extra)
    assert not os.path.exists(tmp_path / "x.tsv")


def test_more_than_one_rank_is_refused(oracle):
    args = SimpleNamespace(model_evidence=["x.tsv"], evidence_ploidy=None, evidence_inbreeding=None)
    with pytest.raises(ValueError, match="single process"):
        cli.model_evidence_settings(args, SAMPLES, 0.1, "AFP", None, 2)
    assert isinstance(cli.model_evidence_settings(args, SAMPLES, 0.1, "AFP", None, 1), application.ModelEvidence)
    vcf = os.path.join(HERE, "mock.input.frequencies.vcf")
    bams = {s: os.path.join(HERE, f) for s, f in zip(SAMPLES, BAMS)}
    acc = application.ModelEvidence(SAMPLES)
    with pytest.raises(ValueError, match="single process"):
        list(application.call_exact(vcf, bams, inbreeding=0.1, calling=oracle, shard=(0, 2), model_evidence=acc))
    with pytest.raises(ValueError, match="samples"):
        list(application.call_exact(vcf, bams, inbreeding=0.1, calling=oracle, model_evidence=application.ModelEvidence(["A"])))
    # and the keyword alone, through the library: the lines of a run without it
    lines = list(application.call_exact(vcf, bams, inbreeding=0.1, prior_frequencies_tag="AFP", calling=oracle, model_evidence=acc))
    assert lines == list(application.call_exact(vcf, bams, inbreeding=0.1, prior_frequencies_tag="AFP", calling=oracle))
    assert acc.records_seen == len(lines) and all(np.isfinite(r["log_evidence"]) for r in acc.table())
