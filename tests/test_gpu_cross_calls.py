"""call-exact --cross-calls from the device: application.CrossCalls over synthetic bi-parental blocks (application.MatrixSource;
tests/cross_reference.py biparental_block) against the host definition on a float64 numpy likelihood backend, field for field
after formatting -- mixed shape groups, unequal parents, a record the library refuses beside records it calls -- and the four side
files of call-exact together in one run on the reference's alignment files."""
import io as _io
import os

import numpy as np
import pytest

from tests import cross_reference as ref

pytestmark = pytest.mark.gpu

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")


def _block(ploidy, **kw):
    from mchap_amd import application

    records, samples, matrices, _ = ref.biparental_block(**kw)
    units = application._exact_units(records, application.MatrixSource(samples, matrices), samples, None, None, False)
    lines = ["\t".join(["chr1", str(u["rec"]["pos"]), ".", "A", ".", ".", "PASS", "AN=0", "GT"] + ["."] * len(samples)) for u in units]
    return units, samples, lines, (lambda s: ploidy.get(s, ploidy[None]))


def _compare(units, samples, lines, ploidy_of, inbreeding_of, parents=("P", "Q"), gamete_error=0.01):
    """The device's lines against the host's, field for field; a CGT that differs must tie with the host's mode within the bound."""
    from mchap_amd import application

    dev = application.CrossCalls(samples, parents, gamete_error=gamete_error)
    got = dev.add_block(units, lines, ploidy_of, inbreeding_of)
    host = application.CrossCalls(samples, parents, gamete_error=gamete_error)
    want = host.add_block(units, lines, ploidy_of, inbreeding_of, ref.NumpyBackend())
    assert set(got) == set(want) and [k for k in got if got[k] is None] == [k for k in want if want[k] is None]
    backend = ref.NumpyBackend()
    for a, b, (ri, unit) in zip(dev.lines, host.lines, enumerate(units)):
        if a == b:
            continue
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:9] == fb[:9]
        for s, ca, cb in zip(samples, fa[9:], fb[9:]):
            if ca == cb:
                continue
            # two genotypes that tie within the bound: the device's has the host's maximal probability, to the bound
            (cgt_a, cgpm_a, clbf_a), (cgt_b, cgpm_b, clbf_b) = ca.rsplit(":", 3)[1:], cb.rsplit(":", 3)[1:]
            assert cgt_a != cgt_b and cgpm_a == cgpm_b and clbf_a == clbf_b
            locus, reads = unit["locus"], unit["reads"]
            H, (P, Q) = len(locus.haplotypes), parents
            llk = {x: backend.genotype_likelihoods(reads[x]["dists"], ploidy_of(x), locus.haplotypes, read_counts=reads[x]["counts"]) for x in (P, Q, s)}
            q = application.cross_prior_unit(llk[P], ploidy_of(P), inbreeding_of(P), llk[Q], ploidy_of(Q), inbreeding_of(Q), H, locus.frequencies,
                                             dev.cross.gamete_error, llk[s])["q"]
            at = int(application._multiset_ranks(np.array([[int(x) for x in cgt_a.split("/")]]))[0])
            assert q.max() - q[at] <= ref.REL * q.max() + ref.FLOOR
    return got, dev.lines


@pytest.mark.parametrize("inbreeding", [None, 0.1], ids=["flat", "dirmul"])
def test_mixed_shape_groups_against_the_host(inbreeding):
    units, samples, lines, ploidy_of = _block({None: 4, "D0": 2, "D1": 6}, depth=40, n_records=4, n_haps=(4, 3, 5, 3), extra={"D0": 2, "D1": 6})
    got, out = _compare(units, samples, lines, ploidy_of, lambda s: inbreeding)
    assert len(got) == 4 * 4 and all(v is not None for v in got.values())
    cols = [ln.split("\t")[9:] for ln in out]
    for row in cols:
        for s, c in zip(samples, row):
            assert (c.rsplit(":", 3)[1:] == [".", ".", "."]) == (s in ("P", "Q", "D0", "D1"))


def test_unequal_parents_and_two_gamete_errors():
    units, samples, lines, ploidy_of = _block({None: 3, "P": 4, "Q": 2}, depth=40, ploidy_p=4, ploidy_q=2, n_records=2)
    got, _ = _compare(units, samples, lines, ploidy_of, lambda s: 0.2, gamete_error=(0.0, 0.2))
    assert len(got) == 2 * 4 and all(v is not None and len(v[0]) == 3 for v in got.values())


def test_a_refused_record_is_null_and_its_neighbours_are_called():
    # ploidy 14 over 200 haplotypes: more than 2^62 genotypes, for the parents and the progeny alike
    units, samples, lines, ploidy_of = _block({None: 14}, depth=20, ploidy_p=14, ploidy_q=14, n_records=3, n_haps=(3, 200, 4), n_pos=8,
                                              n_progeny=2, min_distance=1)
    got, out = _compare(units, samples, lines, ploidy_of, lambda s: None)
    assert all(got[(1, s)] is None for s in ("C0", "C1", "U0")) and all(got[(ri, s)] is not None for ri in (0, 2) for s in ("C0", "C1", "U0"))
    assert all(c.endswith(":.:.:.") for c in out[1].split("\t")[9:]) and "LIMIT" not in out[1]
    assert not any(c.endswith(":.:.:.") for ln in (out[0], out[2]) for s, c in zip(samples, ln.split("\t")[9:]) if s not in ("P", "Q"))


def test_all_four_side_files_in_one_run(tmp_path):
    from mchap_amd import cli

    bams = [os.path.join(HERE, f) for f in ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")]
    base = ["mchap_amd", "call-exact", "--haplotypes", os.path.join(HERE, "mock.input.frequencies.vcf"), "--ploidy", "4", "--bam"] + bams + \
        ["--use-dirmul-prior", "0.1", "AFP", "--estimate-prior-frequencies", "3"]
    cross = ["--cross-parents", "SAMPLE1", "SAMPLE2"]

    def run(extra):
        out = _io.StringIO()
        cli.run(base + extra, out)
        return out.getvalue()

    plain = run([])
    paths = {n: str(tmp_path / n) for n in ("cross.vcf", "e.tsv", "snvs.vcf", "depths.vcf", "alone.vcf")}
    assert run(["--cross-calls", paths["cross.vcf"], "--model-evidence", paths["e.tsv"], "--snv-calls", paths["snvs.vcf"],
                "--allele-depths", paths["depths.vcf"]] + cross) == plain
    assert run(["--cross-calls", paths["alone.vcf"]] + cross) == plain
    assert open(paths["alone.vcf"]).read() == open(paths["cross.vcf"]).read()
    records = [ln.split("\t") for ln in open(paths["cross.vcf"]).read().split("\n") if ln and not ln.startswith("#")]
    assert len(records) >= 3 and all(r[8].endswith(":CGT:CGPM:CLBF") for r in records)
    assert sum(r[6] == "PASS" and not r[11].endswith(":.:.:.") for r in records) >= 2
    assert all(r[9].endswith(":.:.:.") and r[10].endswith(":.:.:.") for r in records)
    assert all(os.path.getsize(paths[n]) > 0 for n in ("e.tsv", "snvs.vcf", "depths.vcf"))
