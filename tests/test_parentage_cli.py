"""call-exact --parentage on the command line, the exact caller replaced by the oracle: the parser's defaults and help, every
argument error, the VCF -- header included -- and the other side files byte for byte what the run writes without the flags, the
table's lines, the flags beside --estimate-prior-frequencies, --model-evidence, --snv-calls, --allele-depths, --cross-calls and
--family-calls.  CPU only."""
import io as _io
import os
from types import SimpleNamespace

import pytest

from mchap_amd import application, cli

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
BAMS = ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")
SAMPLES = ["SAMPLE1", "SAMPLE2", "SAMPLE3"]
PRIOR = ["--use-dirmul-prior", "0.1", "AFP"]
INPUT = os.path.join(HERE, "mock.input.frequencies.vcf")
CANDIDATES = ["--parentage-candidates", "SAMPLE1", "SAMPLE2"]


@pytest.fixture(scope="module")
def oracle():
    from tests.replay_call_exact import OracleBackend

    return OracleBackend()


def _cli(monkeypatch, oracle, extra):
    real = application.call_exact
    monkeypatch.setattr(application, "call_exact", lambda *a, **kw: real(*a, calling=oracle, **kw))
    argv = ["mchap_amd", "call-exact", "--haplotypes", INPUT, "--ploidy", "4", "--bam"] + \
        [os.path.join(HERE, f) for f in BAMS] + ["--report", "AFPRIOR", "AFP"] + extra
    out = _io.StringIO()
    try:
        cli.run(argv, out)
    finally:
        monkeypatch.undo()
    return out.getvalue()


def test_parser_defaults_and_help():
    args = cli.build_parser("call-exact").parse_args([])
    assert args.parentage == [None] and args.parentage_candidates is None and args.parentage_progeny is None
    assert args.parentage_gamete_error == [None] and args.parentage_top == [None]
    args = cli.build_parser("call-exact").parse_args(["--parentage", "p.tsv", "--parentage-candidates", "A", "B", "C", "--parentage-progeny", "D",
                                                       "--parentage-gamete-error", "0.2", "--parentage-top", "3"])
    assert (args.parentage, args.parentage_candidates, args.parentage_progeny, args.parentage_gamete_error, args.parentage_top) == \
        (["p.tsv"], ["A", "B", "C"], ["D"], [0.2], [3])
    helps = {a.option_strings[0]: a.help for a in cli.build_parser("call-exact")._actions if a.option_strings}
    assert cli.PARENTAGE_FLAGS == ("--parentage", "--parentage-candidates", "--parentage-progeny", "--parentage-gamete-error", "--parentage-top")
    for flag in cli.PARENTAGE_FLAGS:
        assert helps[flag].startswith("(not a reference flag)")
        assert flag not in cli.build_parser("call").format_help() and flag not in cli.build_parser("assemble").format_help()
    assert "--parentage FILE" in cli.__doc__


def _settings(ploidy=4, world=1, inbreeding=0.1, tag="AFP", estimate=None, **kw):
    args = SimpleNamespace(**dict(dict(parentage=["x.tsv"], parentage_candidates=["SAMPLE1", "SAMPLE2"], parentage_progeny=None,
                                       parentage_gamete_error=[None], parentage_top=[None]), **kw))
    return cli.parentage_settings(args, SAMPLES, ploidy, inbreeding, tag, estimate, world)


def test_every_argument_error(tmp_path):
    assert _settings(parentage=[None], parentage_candidates=None) is None
    for kw, flag in ((dict(), "--parentage-candidates"), (dict(parentage_candidates=None, parentage_progeny=["SAMPLE3"]), "--parentage-progeny"),
                     (dict(parentage_candidates=None, parentage_gamete_error=[0.1]), "--parentage-gamete-error"),
                     (dict(parentage_candidates=None, parentage_top=[0]), "--parentage-top")):
        with pytest.raises(ValueError, match=flag + " needs --parentage"):
            _settings(parentage=[None], **kw)
    with pytest.raises(ValueError, match="needs --parentage-candidates"):
        _settings(parentage_candidates=None)
    with pytest.raises(ValueError, match="candidate 'NOBODY' is not a sample"):
        _settings(parentage_candidates=["SAMPLE1", "NOBODY"])
    with pytest.raises(ValueError, match="progeny 'NOBODY' is not a sample"):
        _settings(parentage_progeny=["NOBODY"])
    with pytest.raises(ValueError, match="candidate 'SAMPLE1' is named more than once"):
        _settings(parentage_candidates=["SAMPLE1", "SAMPLE2", "SAMPLE1"])
    with pytest.raises(ValueError, match="progeny 'SAMPLE3' is named more than once"):
        _settings(parentage_progeny=["SAMPLE3", "SAMPLE3"])
    with pytest.raises(ValueError, match="candidate 'SAMPLE1' has ploidy 3: an even ploidy"):
        _settings(ploidy={"SAMPLE1": 3, "SAMPLE2": 4, "SAMPLE3": 4})
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="--parentage-gamete-error"):
            _settings(parentage_gamete_error=[bad])
    with pytest.raises(ValueError, match="--parentage-top: N >= 0"):
        _settings(parentage_top=[-1])
    with pytest.raises(ValueError, match="single process"):
        _settings(world=2)
    with pytest.raises(ValueError, match="single process"):
        list(application.call_exact(INPUT, {}, shard=(0, 2), parentage=application.Parentage(SAMPLES, ["SAMPLE1", "SAMPLE2"])))
    table = _settings()
    assert isinstance(table, application.Parentage) and (table.gamete_error, table.top, table.frequency_source) == (0.01, 0, "tag AFP")
    assert table.plan.progeny == ["SAMPLE3"]                                  # every sample that is not a candidate
    assert table.plan.hypotheses["SAMPLE3"] == [("SAMPLE1", "SAMPLE2"), ("SAMPLE1", "."), ("SAMPLE2", "."), (".", ".")]
    table = _settings(parentage_gamete_error=[0.0], parentage_top=[2], parentage_progeny=["SAMPLE2", "SAMPLE3"], estimate=3)
    assert (table.gamete_error, table.top, table.frequency_source) == (0.0, 2, "estimated")
    assert table.plan.hypotheses["SAMPLE2"] == [("SAMPLE1", "."), (".", ".")]   # a candidate and a progeny: never its own parent
    assert _settings(inbreeding=None).frequency_source == "flat"
    assert not os.path.exists(tmp_path / "x.tsv")


def test_the_vcf_is_unchanged_and_the_table_is_written(monkeypatch, oracle, tmp_path, capsys):
    plain = _cli(monkeypatch, oracle, PRIOR)
    path = str(tmp_path / "parentage.tsv")
    assert _cli(monkeypatch, oracle, PRIOR + ["--parentage", path] + CANDIDATES) == plain      # header (its command line too) and records
    cmd = [ln for ln in plain.split("\n") if ln.startswith("##commandline=")][0]
    assert "parentage" not in cmd and "SAMPLE1 SAMPLE2" not in cmd and "--haplotypes" in cmd
    text = open(path).read()
    lines = text.split("\n")
    assert lines[-1] == "" and lines[1].split("\t") == list(application.Parentage.HEADER)
    n_records = len([ln for ln in plain.split("\n")[:-1] if not ln.startswith("#")])
    assert lines[0] == "# mchap_amd call-exact parentage; frequencies: tag AFP; gamete error: 0.01; records: %d" % n_records
    rows = [ln.split("\t") for ln in lines[2:-1]]
    assert len(rows) == 4 and {r[0] for r in rows} == {"SAMPLE3"} and [r[7] for r in rows] == ["1", "2", "3", "4"]
    assert sorted((r[1], r[2]) for r in rows) == sorted([("SAMPLE1", "SAMPLE2"), ("SAMPLE1", "."), ("SAMPLE2", "."), (".", ".")])
    values = [float(r[5]) for r in rows]
    assert values == sorted(values, reverse=True) and float(rows[0][6]) == 0.0 and all(len(r[5].split(".")[1]) == 6 for r in rows)
    assert [r[5] for r in rows if (r[1], r[2]) == (".", ".")] == ["0.000000"]
    assert all(int(r[3]) + int(r[4]) <= n_records and int(r[3]) >= 2 for r in rows)
    # elsewhere on the command line, the "=" form, an abbreviation, the progeny and the defaults named: the same VCF and table
    again = str(tmp_path / "again.tsv")
    assert _cli(monkeypatch, oracle, ["--parentage=" + again, "--parentage-prog", "SAMPLE3", "--parentage-gamete-error", "0.01",
                                      "--parentage-top", "0"] + CANDIDATES + PRIOR) == plain
    assert open(again).read() == text
    top = str(tmp_path / "top.tsv")
    assert _cli(monkeypatch, oracle, PRIOR + ["--parentage", top, "--parentage-top", "1", "--parentage-gamete-error", "0.3"] + CANDIDATES) == plain
    assert len(open(top).read().split("\n")) == 4 and open(top).read().split("\n")[2] != lines[2]
    # together with the estimate (the estimated frequencies are the ones used) and the five other side files, which stay as they are
    est = PRIOR + ["--estimate-prior-frequencies", "3"]
    cross = ["--cross-parents", "SAMPLE1", "SAMPLE2"]
    names = ("e.tsv", "snvs.vcf", "depths.vcf", "cross.vcf", "family.vcf")
    flags = ("--model-evidence", "--snv-calls", "--allele-depths", "--cross-calls", "--family-calls")
    before = [str(tmp_path / ("before_" + n)) for n in names]
    after = [str(tmp_path / ("after_" + n)) for n in names]
    without = _cli(monkeypatch, oracle, est + [x for pair in zip(flags, before) for x in pair] + cross)
    path2 = str(tmp_path / "parentage2.tsv")
    assert _cli(monkeypatch, oracle, est + [x for pair in zip(flags, after) for x in pair] + cross + ["--parentage", path2] + CANDIDATES) == without
    for b, a in zip(before, after):
        assert open(b).read() == open(a).read(), a
    text2 = open(path2).read()
    assert text2.split("\n")[0] == "# mchap_amd call-exact parentage; frequencies: estimated; gamete error: 0.01; records: %d" % n_records
    assert text2 != text
    # the pair's LOG_BF is the sum of the progeny's CLBF column of --cross-calls at the same gamete error, rounded to three decimals
    recs = [ln.split("\t") for ln in open(after[3]).read().split("\n")[:-1] if not ln.startswith("#")]
    clbf = [r[11].rsplit(":", 3)[3] for r in recs]
    pair = [r for r in (ln.split("\t") for ln in text2.split("\n")[2:-1]) if (r[1], r[2]) == ("SAMPLE1", "SAMPLE2")][0]
    if int(pair[4]) == 0:
        total = sum(float(x) for x in clbf if x != ".")
        assert abs(float(pair[5]) - total) <= 5e-4 * len(clbf) + 1e-6
