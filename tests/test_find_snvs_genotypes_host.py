"""find-snvs genotype calls on the host (no GPU): the numpy definition the kernel is held to (snv_genotype_reference.py) against the
oracle's posterior_mode over single-position reads, the --call-* flags, the header with calls, and the GT:GPM:AD columns."""
import os

import numpy as np
import pytest

import snv_genotype_reference as sg

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")


def test_definition_agrees_with_the_oracle_posterior_mode():
    """Seeded cases: ploidy 2/3/4/6, 2-4 alleles, depths 0-39 with alleles left unseen, no prior and (F, None) / (F, frequencies)
    with F in {0, 0.1, 0.5}.  Mode probability to rtol 1e-9 (what test_gpu_exact.py grants mode statistics against the oracle); the
    same mode wherever the definition's two highest posteriors differ by more than 1e-6."""
    from mchap_amd import encoding
    from oracle import binding as ob

    ob.build()
    rng = np.random.default_rng(7)
    called = decided = 0
    for _ in range(400):
        K = int(rng.choice([2, 3, 4, 6]))
        n = int(rng.integers(2, 5))
        d = (rng.integers(0, 40, size=n) * (rng.random(n) < 0.8)).astype(np.int64)
        form = int(rng.integers(0, 3))
        F = float(rng.choice([0.0, 0.1, 0.5]))
        prior = None if form == 0 else (F, None) if form == 1 else (F, rng.dirichlet(np.ones(n)))
        got = sg.mode(d, K, 0.0024, prior)
        if d.sum() == 0:
            assert got is None
            continue
        reads = encoding.encode_read_distributions([n], np.arange(n, dtype=np.int8)[:, None], None, error_rate=0.0024)
        haps = np.arange(n, dtype=np.int8)[:, None]
        alleles, _, mode_prob = ob.posterior_mode(reads, K, haps, read_counts=d, prior=prior)[:3]
        index, prob, gap = got
        called += 1
        np.testing.assert_allclose(prob, mode_prob, rtol=1e-9)
        if gap > 1e-6:
            decided += 1
            assert list(sg.genotypes(n, K)[index]) == [int(a) for a in alleles]
            assert list(ob.index_as_genotype_alleles(index, K)) == [int(a) for a in alleles]
    assert called > 350 and decided > 0.95 * called


def test_definition_edge_cases():
    # error rate 0: an allele that was seen is in the genotype; more alleles seen than copies: no genotype is possible
    index, prob, _ = sg.mode([5, 0, 3], 2, 0.0)
    assert list(sg.genotypes(3, 2)[index]) == [0, 2] and prob == 1.0
    assert sg.mode([5, 1, 3], 2, 0.0) is None
    assert sg.mode([0, 0], 4, 0.0024) is None
    assert sg.mode([4, 4], 2, 0.0024, (0.0, np.array([1.0, 0.0]))) is None
    # depth 60 000: the likelihoods are near -1e5 and the normaliser stays finite
    index, prob, _ = sg.mode([60000, 60000, 0], 4, 0.0024, (0.3, None))
    assert list(sg.genotypes(3, 4)[index]) == [0, 0, 1, 1] and 0.999 < prob <= 1.0
    # flat over the genotypes is not log_genotype_prior with F = 0
    a, b = sg.mode([1, 1], 4, 0.0024), sg.mode([1, 1], 4, 0.0024, (0.0, None))
    assert abs(a[1] - b[1]) > 1e-3


def test_genotype_alleles_unranks_vcf_order():
    from mchap_amd.find_snvs import genotype_alleles

    for K in (1, 2, 3, 4, 6, 15):
        for m in (1, 2, 3, 4):
            g = sg.genotypes(m, K)
            for i in (range(len(g)) if len(g) < 100 else (0, 1, 17, len(g) // 2, len(g) - 1)):
                assert genotype_alleles(i, K) == list(g[i])
                assert genotype_alleles(i, K, refmasked=True) == [a + 1 for a in g[i]]


def test_parser_call_flags_arity_and_defaults(tmp_path):
    from mchap_amd import cli

    p = cli.build_parser("find-snvs")
    d = vars(p.parse_args([]))
    assert d["call_genotypes"] == [None] and d["call_inbreeding"] == [None]
    assert d["call_prior"] == ["FLAT"] and d["call_error_rate"] == [0.0024]
    assert cli.find_snvs_call_settings(p.parse_args([]), ["A", "B"]) is None
    for flag, value, want in (("--call-genotypes", "4", "4"), ("--call-inbreeding", "0.1", "0.1"), ("--call-prior", "ADMF", "ADMF"),
                              ("--call-error-rate", "0.01", 0.01)):
        assert vars(p.parse_args([flag, value]))[flag.lstrip("-").replace("-", "_")] == [want]
        with pytest.raises(SystemExit):
            p.parse_args([flag, value, value])
        with pytest.raises(SystemExit):
            p.parse_args([flag])
    with pytest.raises(SystemExit):
        p.parse_args(["--call-prior", "AFP"])
    with pytest.raises(SystemExit):  # find-snvs still has no --ploidy
        p.parse_args(["--ploidy", "4"])
    # a --call-* flag without --call-genotypes is an error, its default value included
    for other in (["--call-inbreeding", "0.1"], ["--call-prior", "ADMF"], ["--call-prior", "FLAT"], ["--call-error-rate", "0.0024"]):
        with pytest.raises(ValueError, match="needs --call-genotypes"):
            cli.find_snvs_call_settings(p.parse_args(other), ["A", "B"])
    # no prior unless asked for; ADMF alone leaves the inbreeding to mean 0
    s = cli.find_snvs_call_settings(p.parse_args(["--call-genotypes", "4"]), ["A", "B"])
    assert s == dict(ploidy=4, inbreeding=None, frequencies=None, error_rate=0.0024)
    s = cli.find_snvs_call_settings(p.parse_args(["--call-genotypes", "6", "--call-prior", "ADMF", "--call-error-rate", "0"]), ["A", "B"])
    assert s == dict(ploidy=6, inbreeding=None, frequencies="ADMF", error_rate=0.0)
    table = tmp_path / "ploidy.tsv"
    table.write_text("A\t2\nB\t6\n")
    s = cli.find_snvs_call_settings(p.parse_args(["--call-genotypes", str(table), "--call-inbreeding", "0.3"]), ["A", "B"])
    assert s == dict(ploidy={"A": 2, "B": 6}, inbreeding=0.3, frequencies=None, error_rate=0.0024)
    for bad in (["--call-genotypes", "0"], ["--call-genotypes", "4", "--call-inbreeding", "1.0"],
                ["--call-genotypes", "4", "--call-error-rate", "1.5"]):
        with pytest.raises(ValueError):
            cli.find_snvs_call_settings(p.parse_args(bad), ["A", "B"])


def test_header_declares_gpm_only_with_calls():
    from mchap_amd import io, vcfheader

    want = [ln.rstrip("\n") for ln in open(os.path.join(HERE, "simple.output.basis.vcf")) if ln.startswith("#")]
    contigs = io.Reference(os.path.join(HERE, "simple.fasta")).contigs
    args = (["mchap_amd", "find-snvs"], "simple.fasta", ["SAMPLE1", "SAMPLE2", "SAMPLE3"], contigs)
    plain = vcfheader.find_snvs_header_lines(*args)
    assert plain == vcfheader.find_snvs_header_lines(*args, genotypes=False)
    exempt = ("##fileDate", "##source", "##commandline")
    assert [ln for ln in plain if not ln.startswith(exempt)] == [ln for ln in want if not ln.startswith(exempt)]
    calling = vcfheader.find_snvs_header_lines(*args, genotypes=True)
    extra = '##FORMAT=<ID=GPM,Number=1,Type=Float,Description="Genotype posterior mode probability">'
    assert extra not in plain and calling.count(extra) == 1
    assert [ln for ln in calling if ln != extra] == plain
    assert calling.index(extra) == calling.index(next(ln for ln in calling if ln.startswith("##FORMAT=<ID=GT,"))) + 1


def test_format_records_with_calls():
    from mchap_amd.find_snvs import format_records

    flags = np.array([
        sg.record_flag([0, 2, 1, 3], [1, 0, 1, 0]),   # A>G
        sg.record_flag([1, 3, 0, 2], [0, 0, 1, 1]),   # C>T,G with the reference masked: the enumerated alleles are VCF 1 and 2
        sg.record_flag([3, 0, 1, 2], [1, 1, 0, 1]),   # T>A,C: tri-allelic
    ])
    depth = np.array([[[9, 0, 8, 1], [20, 0, 0, 0], [0, 0, 0, 0]],
                      [[0, 1, 7, 6], [0, 0, 0, 12], [1, 0, 3, 0]],
                      [[5, 4, 0, 6], [0, 9, 0, 0], [2, 0, 0, 30]]])
    admf = np.array([[0.6, 0.0, 0.4, 0.0], [0.0, 0.0, 0.3, 0.7], [0.25, 0.3, 0.0, 0.45]])
    ploidy = [2, 4, 6]
    # indices over the enumerated alleles: row 1 has two (G and T in VCF order T, G)
    gt = np.array([[1, 0, -1], [1, 0, 6], [4, 14, 0]])
    gpm = np.array([[0.99951, 1.0, np.nan], [0.5, 0.87649, 0.3334], [0.7, 0.99999, 0.12]])
    lines = format_records(["c"] * 3, [9, 19, 29], depth, flags, admf, gt_index=gt, gpm=gpm, ploidy=ploidy)
    rows = [ln.split("\t") for ln in lines]
    assert [r[:5] for r in rows] == [["c", "10", ".", "A", "G"], ["c", "20", ".", "C", "T,G"], ["c", "30", ".", "T", "A,C"]]
    assert [r[7] for r in rows] == ["AD=29,8;ADMF=0.6,0.4", "REFMASKED;AD=1,18,10;ADMF=0,0.7,0.3", "AD=36,7,13;ADMF=0.45,0.25,0.3"]
    assert all(r[8] == "GT:GPM:AD" for r in rows)
    assert rows[0][9:] == ["0/1:1:9,8", "0/0/0/0:1:20,0", "./././././.:.:0,0"]
    assert rows[1][9:] == ["1/2:0.5:1,6,7", "1/1/1/1:0.876:0,12,0", "2/2/2/2/2/2:0.333:0,0,3"]
    assert rows[2][9:] == ["1/2:0.7:6,5,4", "2/2/2/2:1:0,0,9", "0/0/0/0/0/0:0.12:30,2,0"]
    # one ploidy for all samples; and without calls the lines are what they were
    same = format_records(["c"] * 3, [9, 19, 29], depth, flags, admf, gt_index=np.zeros((3, 3), int), gpm=np.full((3, 3), 0.25), ploidy=3)
    assert same[1].split("\t")[9:] == ["1/1/1:0.25:1,6,7", "1/1/1:0.25:0,12,0", "1/1/1:0.25:0,0,3"]
    plain = format_records(["c"] * 3, [9, 19, 29], depth, flags, admf)
    assert [ln.split("\t")[8:] for ln in plain] == [["GT:AD", ".:9,8", ".:20,0", ".:0,0"], ["GT:AD", ".:1,6,7", ".:0,12,0", ".:0,0,3"],
                                                   ["GT:AD", ".:6,5,4", ".:0,0,9", ".:30,2,0"]]
    assert [ln.split("\t")[:8] for ln in plain] == [r[:8] for r in rows]
    with pytest.raises(ValueError):
        format_records(["c"] * 3, [9, 19, 29], depth, flags, admf, gt_index=gt)
