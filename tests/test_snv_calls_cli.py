"""call-exact --snv-calls / --snv-report and `atomize` on the command line, the exact caller replaced by the oracle: the parser's
defaults, the flag errors, the SNV file, and the VCF -- header included -- byte for byte what the run writes without the flags.
CPU only."""
import io as _io
import os
from types import SimpleNamespace

import pytest

from mchap_amd import application, cli

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
BAMS = ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")
SAMPLES = ["SAMPLE1", "SAMPLE2", "SAMPLE3"]
PRIOR = ["--use-dirmul-prior", "0.1", "AFP"]


@pytest.fixture(scope="module")
def oracle():
    from tests.replay_call_exact import OracleBackend

    return OracleBackend()


def _cli(monkeypatch, oracle, extra):
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


def test_parser_defaults_and_help():
    assert "atomize" in cli.PROGRAMS
    args = cli.build_parser("call-exact").parse_args([])
    assert args.snv_calls == [None] and args.snv_report is None
    args = cli.build_parser("call-exact").parse_args(["--snv-calls", "s.vcf", "--snv-report", "GP"])
    assert args.snv_calls == ["s.vcf"] and args.snv_report == ["GP"]
    with pytest.raises(SystemExit):
        cli.build_parser("call-exact").parse_args(["--snv-calls", "s.vcf", "--snv-report", "GL"])
    helps = {a.option_strings[0]: a.help for a in cli.build_parser("call-exact")._actions if a.option_strings}
    for flag in cli.SNV_FLAGS:
        assert helps[flag].startswith("(not a reference flag)")
        assert flag not in cli.build_parser("call").format_help() and flag not in cli.build_parser("assemble").format_help()
    assert cli.EVIDENCE_FLAGS == ("--model-evidence", "--evidence-ploidy", "--evidence-inbreeding")
    assert [a.option_strings for a in cli.build_parser("atomize")._actions if a.option_strings and a.dest != "help"] == [["--haplotypes"]]


def test_the_vcf_is_unchanged_and_the_snv_file_is_written(monkeypatch, oracle, tmp_path):
    plain = _cli(monkeypatch, oracle, PRIOR)
    path = str(tmp_path / "snvs.vcf")
    assert _cli(monkeypatch, oracle, PRIOR + ["--snv-calls", path]) == plain     # header (its command line too) and records
    text = open(path).read()
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0] == "##fileformat=VCFv4.3"
    cmd = [ln for ln in lines if ln.startswith("##commandline=")][0]
    assert "--snv-calls" not in cmd and "--haplotypes" in cmd
    assert [ln for ln in lines if ln.startswith("##contig=")] == [ln for ln in plain.split("\n") if ln.startswith("##contig=")]
    assert [ln for ln in lines if ln.startswith("#CHROM")][0].split("\t")[8:] == ["FORMAT"] + SAMPLES
    records = [ln.split("\t") for ln in lines[:-1] if not ln.startswith("#")]
    assert len(records) >= 5 and all(r[8] == "GT:GQ:PQ:DP:DS" and r[2].split("_SNV")[1].isdigit() for r in records)
    # with GP, in other places of the command line, "=" forms and abbreviations: still the same VCF; the SNV file gains a field
    gp = str(tmp_path / "gp.vcf")
    assert _cli(monkeypatch, oracle, ["--snv-calls=" + gp] + PRIOR + ["--snv-rep", "GP"]) == plain
    gp_records = [ln.split("\t") for ln in open(gp).read().split("\n")[:-1] if not ln.startswith("#")]
    assert [r[8] for r in gp_records] == ["GT:GQ:PQ:DP:DS:GP"] * len(records)
    assert [[c.rsplit(":", 1)[0] for c in r[9:]] for r in gp_records] == [r[9:] for r in records]
    assert '##FORMAT=<ID=GP,Number=G,Type=Float,Description="Genotype posterior probabilities">' in open(gp).read()
    # together with the estimate (the posterior uses the estimated frequencies) and with the model evidence
    est = PRIOR + ["--estimate-prior-frequencies", "3"]
    with_estimate = _cli(monkeypatch, oracle, est)
    path2, table = str(tmp_path / "snvs2.vcf"), str(tmp_path / "e.tsv")
    assert _cli(monkeypatch, oracle, est + ["--snv-calls", path2, "--model-evidence", table]) == with_estimate
    records2 = [ln.split("\t") for ln in open(path2).read().split("\n")[:-1] if not ln.startswith("#")]
    assert [r[:5] for r in records2] == [r[:5] for r in records] and [r[7] for r in records2] != [r[7] for r in records]
    assert os.path.exists(table)
    # `atomize` of the run's own VCF through cli.run: the SNV file but for GQ, DS and ACP
    main = str(tmp_path / "main.vcf")
    with open(main, "w") as f:
        f.write(plain)
    out = _io.StringIO()
    n = cli.run(["mchap_amd", "atomize", "--haplotypes", main], out)
    atomized = [ln.split("\t") for ln in out.getvalue().split("\n")[:-1] if not ln.startswith("#")]
    assert n == len(atomized) == len(records)
    strip = lambda r: r[:7] + [";".join(kv for kv in r[7].split(";") if not kv.startswith("ACP="))] + [[c.split(":")[0]] + c.split(":")[2:4] for c in r[9:]]
    assert [strip(r) for r in atomized] == [strip(r) for r in records]
    assert all(c.split(":")[1] == "." for r in atomized for c in r[9:])
    assert '##commandline="mchap_amd atomize --haplotypes %s"' % main in out.getvalue()


def test_atomize_warns_and_needs_its_flag(capsys):
    out = _io.StringIO()
    cli.run(["mchap_amd", "atomize", "--haplotypes", os.path.join(HERE, "simple.output.mixed_depth.assemble.counts.vcf")], out)
    assert "experimental" in capsys.readouterr().err
    want = open(os.path.join(HERE, "simple.output.mixed_depth.assemble.counts.atomize.vcf")).read().split("\n")
    varying = ("##fileDate", "##source", "##commandline")
    assert [ln for ln in out.getvalue().split("\n") if not ln.startswith(varying)] == [ln for ln in want if not ln.startswith(varying)]
    with pytest.raises(ValueError, match="--haplotypes is required"):
        cli.run(["mchap_amd", "atomize"], _io.StringIO())


def test_errors(monkeypatch, oracle, tmp_path):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="--snv-report needs --snv-calls"):
        _cli(monkeypatch, oracle, PRIOR + ["--snv-report", "GP"])
    args = SimpleNamespace(snv_calls=["x.vcf"], snv_report=None, haplotypes=[os.path.join(HERE, "mock.input.frequencies.vcf")])
    with pytest.raises(ValueError, match="single process"):
        cli.snv_calls_settings(args, SAMPLES, 2, ["mchap_amd"])
    assert isinstance(cli.snv_calls_settings(args, SAMPLES, 1, ["mchap_amd"]), application.SnvCalls)
    assert cli.snv_calls_settings(SimpleNamespace(snv_calls=[None], snv_report=None), SAMPLES, 1, []) is None
    assert not os.path.exists(tmp_path / "x.vcf")
