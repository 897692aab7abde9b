"""call-exact --cross-calls on the command line, the exact caller replaced by the oracle: the parser's defaults and help, every
argument error, the VCF -- header included -- byte for byte what the run writes without the flags, the file's header and columns,
the flags beside --estimate-prior-frequencies, --model-evidence, --snv-calls and --allele-depths.  CPU only."""
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
CROSS = ["--cross-parents", "SAMPLE1", "SAMPLE2"]
IDS = ["CGT", "CGPM", "CLBF"]


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


def _records(text):
    return [ln.split("\t") for ln in text.split("\n")[:-1] if not ln.startswith("#")]


def _declared(line):
    return any(line.startswith("##FORMAT=<ID=%s," % i) for i in IDS)


def test_parser_defaults_and_help():
    args = cli.build_parser("call-exact").parse_args([])
    assert args.cross_calls == [None] and args.cross_parents is None and args.cross_progeny is None and args.gamete_error is None
    args = cli.build_parser("call-exact").parse_args(["--cross-calls", "c.vcf", "--cross-parents", "A", "B", "--cross-progeny", "C", "D",
                                                       "--gamete-error", "0.01", "0.2"])
    assert (args.cross_calls, args.cross_parents, args.cross_progeny, args.gamete_error) == (["c.vcf"], ["A", "B"], ["C", "D"], [0.01, 0.2])
    helps = {a.option_strings[0]: a.help for a in cli.build_parser("call-exact")._actions if a.option_strings}
    assert cli.CROSS_FLAGS == ("--cross-calls", "--cross-parents", "--cross-progeny", "--gamete-error")
    for flag in cli.CROSS_FLAGS:
        assert helps[flag].startswith("(not a reference flag)")
        assert flag not in cli.build_parser("call").format_help() and flag not in cli.build_parser("assemble").format_help()


def _settings(ploidy=4, world=1, **kw):
    args = SimpleNamespace(**dict(dict(cross_calls=["x.vcf"], cross_parents=["SAMPLE1", "SAMPLE2"], cross_progeny=None, gamete_error=None), **kw))
    return cli.cross_calls_settings(args, SAMPLES, ploidy, world, ["##fileformat=VCFv4.3"])


def test_every_argument_error(tmp_path):
    assert _settings(cross_calls=[None], cross_parents=None) is None
    for kw, flag in ((dict(cross_parents=["A", "B"]), "--cross-parents"), (dict(cross_parents=None, cross_progeny=["A"]), "--cross-progeny"),
                     (dict(cross_parents=None, gamete_error=[0.1]), "--gamete-error")):
        with pytest.raises(ValueError, match=flag + " needs --cross-calls"):
            _settings(cross_calls=[None], **kw)
    with pytest.raises(ValueError, match="needs --cross-parents"):
        _settings(cross_parents=None)
    with pytest.raises(ValueError, match="not a sample"):
        _settings(cross_parents=["SAMPLE1", "NOBODY"])
    with pytest.raises(ValueError, match="not a sample"):
        _settings(cross_progeny=["NOBODY"])
    with pytest.raises(ValueError, match="one sample"):
        _settings(cross_parents=["SAMPLE1", "SAMPLE1"])
    with pytest.raises(ValueError, match="even ploidy"):
        _settings(ploidy={"SAMPLE1": 3, "SAMPLE2": 4, "SAMPLE3": 4})
    with pytest.raises(ValueError, match="progeny 'SAMPLE3' has ploidy 4, the cross gives 3"):
        _settings(ploidy={"SAMPLE1": 2, "SAMPLE2": 4, "SAMPLE3": 4}, cross_progeny=["SAMPLE3"])
    with pytest.raises(ValueError, match="single process"):
        _settings(world=2)
    for bad in ([1.5], [-0.1], [float("nan")], [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError, match="--gamete-error"):
            _settings(gamete_error=bad)
    calls = _settings(gamete_error=[0.0, 0.2])
    assert isinstance(calls, application.CrossCalls) and calls.cross.gamete_error == (0.0, 0.2)
    assert _settings().cross.gamete_error == (0.01, 0.01)
    # the default progeny: every other sample of ploidy t_P + t_Q
    assert _settings().cross.resolve(SAMPLES, lambda s: 4)[2] == ["SAMPLE3"]
    assert _settings(ploidy={"SAMPLE1": 2, "SAMPLE2": 4, "SAMPLE3": 4}).cross.resolve(SAMPLES, {"SAMPLE1": 2, "SAMPLE2": 4, "SAMPLE3": 4}.get)[2] == []
    assert not os.path.exists(tmp_path / "x.vcf")
    with pytest.raises(ValueError, match="single process"):
        list(application.call_exact(INPUT, {}, shard=(0, 2), cross_calls=application.CrossCalls(SAMPLES, ("SAMPLE1", "SAMPLE2"))))


def test_the_vcf_is_unchanged_and_the_file_is_written(monkeypatch, oracle, tmp_path):
    plain = _cli(monkeypatch, oracle, PRIOR)
    path = str(tmp_path / "cross.vcf")
    assert _cli(monkeypatch, oracle, PRIOR + ["--cross-calls", path] + CROSS) == plain         # header (its command line too) and records
    text = open(path).read()
    lines, plain_lines = text.split("\n"), plain.split("\n")
    assert lines[-1] == ""
    head, plain_head = [ln for ln in lines if ln.startswith("#")], [ln for ln in plain_lines if ln.startswith("#")]
    assert [ln for ln in head if not _declared(ln)] == plain_head
    added = [ln for ln in head if _declared(ln)]
    assert [ln.split(",")[0][len("##FORMAT=<ID="):] for ln in added] == IDS and all("Number=1" in ln for ln in added)
    last = max(i for i, ln in enumerate(head) if ln.startswith("##FORMAT=<"))
    assert head[last - 2:last + 1] == added and "SAMPLE1 and SAMPLE2" in added[0]
    cmd = [ln for ln in head if ln.startswith("##commandline=")][0]
    assert not any(flag in cmd for flag in cli.CROSS_FLAGS) and "SAMPLE1 SAMPLE2" not in cmd and "--haplotypes" in cmd
    records, plain_records = _records(text), _records(plain)
    assert len(records) == len(plain_records) >= 3
    called = 0
    for r, p in zip(records, plain_records):
        assert r[:8] == p[:8] and r[8] == p[8] + ":CGT:CGPM:CLBF" and [c.rsplit(":", 3)[0] for c in r[9:]] == p[9:]
        fields = [c.rsplit(":", 3)[1:] for c in r[9:]]
        assert fields[0] == fields[1] == [".", ".", "."]                                    # the parents
        if r[6] != "PASS":
            assert fields[2] == [".", ".", "."]
        else:
            cgt, cgpm, clbf = fields[2]
            assert len(cgt.split("/")) == 4 and 0.0 <= float(cgpm) <= 1.0 and len(clbf.split(".")[1]) == 3
            called += 1
    assert called >= 2
    # elsewhere on the command line, the "=" form, an abbreviation, the progeny and the default error named: the same VCF and file
    again = str(tmp_path / "again.vcf")
    assert _cli(monkeypatch, oracle, ["--cross-c=" + again, "--cross-progeny", "SAMPLE3", "--gamete-error", "0.01"] + CROSS + PRIOR) == plain
    assert open(again).read() == text
    other = str(tmp_path / "other.vcf")
    assert _cli(monkeypatch, oracle, PRIOR + ["--cross-calls", other, "--gamete-error", "0.01", "0.5"] + CROSS) == plain
    assert open(other).read() != text
    # together with the estimate (the estimated frequencies are the ones used) and the three other side files
    est = PRIOR + ["--estimate-prior-frequencies", "3"]
    with_estimate = _cli(monkeypatch, oracle, est)
    path2, table, snvs, depths = (str(tmp_path / n) for n in ("cross2.vcf", "e.tsv", "snvs.vcf", "depths.vcf"))
    assert _cli(monkeypatch, oracle, est + ["--cross-calls", path2, "--model-evidence", table, "--snv-calls", snvs, "--allele-depths", depths]
                + CROSS) == with_estimate
    records2 = _records(open(path2).read())
    assert [r[:5] for r in records2] == [r[:5] for r in records] and "EMIT=" in records2[0][7]
    assert [r[9:] for r in records2] != [r[9:] for r in records]
    assert os.path.exists(table) and os.path.exists(snvs) and os.path.exists(depths)
    assert [ln for ln in open(path2).read().split("\n") if ln.startswith("#") and not _declared(ln)] == \
        [ln for ln in with_estimate.split("\n") if ln.startswith("#")]
    alone = str(tmp_path / "depths_alone.vcf")
    _cli(monkeypatch, oracle, est + ["--allele-depths", alone])
    assert open(alone).read() == open(depths).read()                    # the other side files do not depend on the flags either
