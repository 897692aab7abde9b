"""`atomize` (mchap_amd/atomize.py) against the reference's three golden pairs, byte for byte apart from the date, source and
command lines; the allele indexing and the float texts with the reference's own expected values (its test_application_atomize.py,
as data); the compressed input; the cases the goldens are silent on.  CPU only."""
import gzip
import io as _io
import os

import numpy as np
import pytest

from mchap_amd import atomize

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
PAIRS = [("simple.output.mixed_depth.assemble%s.vcf" % v, "simple.output.mixed_depth.assemble%s.atomize.vcf" % v)
         for v in ("", ".counts", ".frequencies")]
VARYING = ("##fileDate", "##source", "##commandline")


def _atomized(path):
    out = _io.StringIO()
    n = atomize.atomize_vcf(path, out)
    lines = out.getvalue().split("\n")
    assert lines[-1] == "" and n == len([ln for ln in lines[:-1] if not ln.startswith("#")])
    return lines[:-1]


@pytest.mark.parametrize("input_vcf, output_vcf", PAIRS)
def test_the_reference_goldens(input_vcf, output_vcf):
    got = _atomized(os.path.join(HERE, input_vcf))
    want = open(os.path.join(HERE, output_vcf)).read().split("\n")[:-1]
    assert len(got) == len(want) and len([ln for ln in want if not ln.startswith("#")]) == 5
    for g, w in zip(got, want):
        if w.startswith(VARYING):
            assert g.startswith(w.split("=", 1)[0] + "=")
        else:
            assert g == w


def test_a_compressed_input(tmp_path):
    plain = os.path.join(HERE, PAIRS[1][0])
    packed = str(tmp_path / "in.vcf.gz")
    with gzip.open(packed, "wb") as f:
        f.write(open(plain, "rb").read())
    keep = lambda lines: [ln for ln in lines if not ln.startswith("##commandline")]
    assert keep(_atomized(packed)) == keep(_atomized(plain))


SNVS = np.array([["A", "C", "A", "C"], ["A", "C", "G", "C"], ["A", "T", "T", "G"]])


def test_format_snv_alleles():
    refs, alts, n_alts = atomize.format_snv_alleles(SNVS)
    np.testing.assert_array_equal(refs, ["A", "C", "A", "C"])
    np.testing.assert_array_equal(alts, ["", "T", "G,T", "G"])
    np.testing.assert_array_equal(n_alts, [0, 1, 2, 1])


def test_snv_allele_indices():
    np.testing.assert_array_equal(atomize.snv_allele_indices(SNVS), [[0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 2, 1]])
    # first appearance over the haplotypes, not alphabetical order
    np.testing.assert_array_equal(atomize.snv_allele_indices(np.array([["T"], ["G"], ["T"], ["A"], ["G"]]))[:, 0], [0, 1, 0, 2, 1])


def _floats():
    floats = np.arange(60).reshape(5, 3, 4) / 15
    floats[1] = np.nan
    floats[3, 1] = [0.0, 1.0, np.nan, 1.1]
    return floats


def test_format_allele_floats__R():
    actual = atomize.format_allele_floats(_floats(), np.array([1, 1, 2, 3]))
    expect = np.array([["0,0.067", "0.267,0.333", "0.533,0.6"], [".,.", ".,.", ".,."],
                       ["1.6,1.667,1.733", "1.867,1.933,2", "2.133,2.2,2.267"],
                       ["2.4,2.467,2.533,2.6", "0,1,.,1.1", "2.933,3,3.067,3.133"]])
    np.testing.assert_array_equal(actual, expect)


def test_format_allele_floats__A():
    actual = atomize.format_allele_floats(_floats()[:, :, 1:], np.array([1, 1, 2, 3]), length="A")
    expect = np.array([["0.067", "0.333", "0.6"], [".", ".", "."], ["1.667,1.733", "1.933,2", "2.2,2.267"],
                       ["2.467,2.533,2.6", "1,.,1.1", "3,3.067,3.133"]])
    np.testing.assert_array_equal(actual, expect)
    np.testing.assert_array_equal(atomize.format_allele_floats(np.array([[10.0, 0.0006, 2.0], [np.nan, 20.0, 0.25]]), [2, 1]),
                                  ["10,0.001,2", ".,20"])   # (two dimensions: one text per SNV)
    with pytest.raises(ValueError):
        atomize.format_allele_floats(np.zeros(3), [1])


def test_genotype_rank():
    assert [atomize.genotype_rank(g) for g in ((0, 0), (0, 1), (1, 1), (0, 2), (2, 1), (2, 2))] == [0, 1, 2, 3, 4, 5]
    assert atomize.genotype_rank((3,) * 15) == 815


HEADER = "\n".join(["##fileformat=VCFv4.3", "##contig=<ID=C1,length=100>",
                    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB"]) + "\n"


def _records(tmp_path, *lines):
    path = str(tmp_path / "t.vcf")
    with open(path, "w") as f:
        f.write(HEADER + "".join(ln + "\n" for ln in lines))
    return [ln.split("\t") for ln in _atomized(path) if not ln.startswith("#")]


def test_where_the_goldens_are_silent(tmp_path):
    recs = _records(
        tmp_path,
        # no SNV: nothing is written
        "C1\t5\tr0\tACGT\t.\t.\tPASS\tAN=4;SNVPOS=.\tGT:SQ\t0/0:60\t0/0:60",
        # an SNV at which no haplotype differs from REF (position 1): the empty ALT; SNVDP -> DP; a null call; no id
        "C1\t10\t.\tACGT\tACTT,AGTA\t.\tPASS\tSNVPOS=1,3,4\tGT:SQ:SNVDP:AFP\t0/1/2/2:13:7,8,9:0.25,0.25,0.5\t./.:.:2,3,4:0.5,0.5,0",
        # SNVDP missing for a sample: the reference's float texts
        "C1\t20\tr2\tAC\tAT\t.\tPASS\tSNVPOS=2\tGT:SQ:SNVDP\t0|1:5:6\t1/1:7")
    assert [r[:5] for r in recs] == [["C1", "10", ".", "A", ""], ["C1", "12", ".", "G", "T"], ["C1", "13", ".", "T", "A"],
                                     ["C1", "21", "r2_SNV1", "C", "T"]]
    assert recs[0][7:] == ["AC=;ACP=6;DP=9;PS=10", "GT:GQ:PQ:DP:DS", "0|0|0|0:.:13:7:", ".|.:.:.:2:"]
    assert recs[1][7:] == ["AC=3;ACP=2,4;DP=11;PS=10", "GT:GQ:PQ:DP:DS", "0|1|1|1:.:13:8:3", ".|.:.:.:3:1"]
    assert recs[2][7:] == ["AC=2;ACP=4,2;DP=13;PS=10", "GT:GQ:PQ:DP:DS", "0|0|1|1:.:13:9:2", ".|.:.:.:4:0"]
    assert recs[3][7:] == ["AC=3;ACP=.,.;DP=.;PS=20", "GT:GQ:PQ:DP:DS", "0|1:.:5:6.0:.", "1|1:.:7:.:."]
