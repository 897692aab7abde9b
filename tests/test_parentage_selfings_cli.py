"""call-exact --parentage --parentage-selfings on the command line, the exact caller replaced by the oracle: the flag's default,
help and doc, its argument error, the VCF -- header included -- byte for byte what the run writes without it, the table without
the flag byte for byte today's, and with it the marker of the '#' line and the selfing rows.  CPU only."""
from types import SimpleNamespace

import pytest

from mchap_amd import application, cli
from tests.test_parentage_cli import CANDIDATES, PRIOR, SAMPLES, _cli, oracle  # noqa: F401


def test_the_flag_its_help_and_the_doc():
    parser = cli.build_parser("call-exact")
    assert parser.parse_args([]).parentage_selfings is False
    assert parser.parse_args(["--parentage", "p.tsv", "--parentage-candidates", "A", "--parentage-selfings"]).parentage_selfings is True
    helps = {a.option_strings[0]: a.help for a in parser._actions if a.option_strings}
    assert cli.PARENTAGE_SELFING_FLAGS == ("--parentage-selfings",) and "--parentage-selfings" not in cli.PARENTAGE_FLAGS
    assert helps["--parentage-selfings"].startswith("(not a reference flag)")
    assert "--parentage-selfings" not in cli.build_parser("call").format_help()
    assert "[--parentage-selfings]" in cli.__doc__


def _settings(**kw):
    args = SimpleNamespace(**dict(dict(parentage=["x.tsv"], parentage_candidates=["SAMPLE1", "SAMPLE2"], parentage_progeny=None,
                                       parentage_gamete_error=[None], parentage_top=[None]), **kw))
    return cli.parentage_settings(args, SAMPLES, 4, 0.1, "AFP", None, 1)


def test_the_argument_error_and_the_settings():
    with pytest.raises(ValueError, match="--parentage-selfings needs --parentage"):
        _settings(parentage=[None], parentage_candidates=None, parentage_selfings=True)
    assert _settings(parentage=[None], parentage_candidates=None, parentage_selfings=False) is None
    assert _settings().selfings is False                                         # a namespace without the attribute
    table = _settings(parentage_selfings=True)
    assert table.selfings and table.plan.hypotheses["SAMPLE3"] == [("SAMPLE1", "SAMPLE2"), ("SAMPLE1", "SAMPLE1"), ("SAMPLE2", "SAMPLE2"),
                                                                  ("SAMPLE1", "."), ("SAMPLE2", "."), (".", ".")]
    with pytest.raises(ValueError, match="two parents are one sample"):          # --cross-parents P P stays the error it is
        application.Cross(("SAMPLE1", "SAMPLE1")).resolve(SAMPLES, lambda s: 4)


def test_the_vcf_is_unchanged_and_the_table_gains_the_selfing_rows(monkeypatch, oracle, tmp_path):  # noqa: F811
    plain = _cli(monkeypatch, oracle, PRIOR)
    without, path = str(tmp_path / "without.tsv"), str(tmp_path / "with.tsv")
    assert _cli(monkeypatch, oracle, PRIOR + ["--parentage", without] + CANDIDATES) == plain
    assert _cli(monkeypatch, oracle, PRIOR + ["--parentage", path, "--parentage-selfings"] + CANDIDATES) == plain   # header too
    assert _cli(monkeypatch, oracle, ["--parentage-self", "--parentage", str(tmp_path / "again.tsv")] + CANDIDATES + PRIOR) == plain
    cmd = [ln for ln in plain.split("\n") if ln.startswith("##commandline=")][0]
    assert "selfings" not in cmd and "parentage" not in cmd
    assert open(str(tmp_path / "again.tsv")).read() == open(path).read()
    old, new = open(without).read().split("\n"), open(path).read().split("\n")
    assert "selfings" not in old[0] and new[0] == old[0] + "; selfings: yes" and new[1] == old[1]
    rows = [ln.split("\t") for ln in new[2:-1]]
    assert len(rows) == 6 and [r[7] for r in rows] == ["1", "2", "3", "4", "5", "6"]
    assert sorted((r[1], r[2]) for r in rows) == sorted([("SAMPLE1", "SAMPLE2"), ("SAMPLE1", "SAMPLE1"), ("SAMPLE2", "SAMPLE2"),
                                                          ("SAMPLE1", "."), ("SAMPLE2", "."), (".", ".")])
    # the rows the table had keep their LOG_BF, RECORDS and SKIPPED: the selfing rows are added, nothing else moves
    was = {(r[1], r[2]): r[3:6] for r in (ln.split("\t") for ln in old[2:-1])}
    assert all(r[3:6] == was[(r[1], r[2])] for r in rows if (r[1], r[2]) in was) and len(was) == 4
    values = [float(r[5]) for r in rows]
    assert values == sorted(values, reverse=True) and all(v == v for v in values)
