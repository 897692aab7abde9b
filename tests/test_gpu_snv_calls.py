"""call-exact --snv-calls on the device, end to end on the reference's files (tetraploid, three samples): the arrays
SnvCalls.add_block returns against the definition (application.snv_posteriors_host) on the library's own float64 likelihoods, the
SNV file's text against the definition's, and the record lines with and without the writer -- under the flat prior, the
Dirichlet-multinomial prior and after the frequency estimate, record by record and on the block path."""
import os
from math import comb

import numpy as np
import pytest

from mchap_amd import application, atomize
from tests import snv_posterior_reference as ref
from tests.test_gpu_model_evidence import Calling64   # (the oracle returns the reference's float32 likelihoods: 1e-7 apart)

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
SAMPLES = ["SAMPLE1", "SAMPLE2", "SAMPLE3"]
BAMS = ("simple.sample1.bam", "simple.sample2.deep.bam", "simple.sample3.bam")
VCF = os.path.join(HERE, "mock.input.frequencies.vcf")
PRIORS = {"flat": dict(), "dirmul": dict(inbreeding=0.1, prior_frequencies_tag="AFP"),
          "estimate": dict(inbreeding=0.1, prior_frequencies_tag="AFP", estimate_frequencies=5)}


@pytest.fixture(scope="module")
def source():
    """The golden job's pileups as a MatrixSource (keyed by (record id, sample))."""
    bams = application.ReadSource({s: os.path.join(HERE, f) for s, f in zip(SAMPLES, BAMS)})
    _, records = application.read_vcf(VCF)
    units = application._exact_units(records, bams, SAMPLES, "AFP", None, False)
    matrices = {(u["locus"].name, s): (u["reads"][s]["chars"], np.zeros(u["reads"][s]["chars"].shape, dtype=np.int16)) for u in units for s in SAMPLES}
    return application.MatrixSource(SAMPLES, matrices)


def _numbers(text):
    return [np.nan if x == "." else float(x) for x in text.split(",")]


@pytest.mark.parametrize("block_path", [False, True])
@pytest.mark.parametrize("prior", list(PRIORS))
def test_the_program_against_the_definition(prior, block_path, source):
    kw = dict(ploidy=4, report=("ACP",), block_path=block_path, **PRIORS[prior])
    plain = list(application.call_exact(VCF, source, **kw))
    snv = application.SnvCalls(SAMPLES, atomize.vcf_contig_lines(VCF), report=("GP",))
    assert list(application.call_exact(VCF, source, snv_calls=snv, **kw)) == plain             # the record lines are identical
    assert len(snv.lines) >= 5
    # the same block by hand: the device's arrays against the definition on the library's float64 likelihoods
    _, records = application.read_vcf(VCF)
    tag = PRIORS[prior].get("prior_frequencies_tag")
    units = application._exact_units(records, source, SAMPLES, tag, None, block_path)
    ploidy_of, inbreeding_of = (lambda s: 4), (lambda s: PRIORS[prior].get("inbreeding"))
    if prior == "estimate":
        application.estimate_prior_frequencies(units, SAMPLES, ploidy_of, inbreeding_of, 5)
    dev = application.SnvCalls(SAMPLES, atomize.vcf_contig_lines(VCF), report=("GP",))
    got = dev.add_block(units, plain, ploidy_of, inbreeding_of)
    assert dev.lines == snv.lines                                                             # the program's file is this file
    host = application.SnvCalls(SAMPLES, atomize.vcf_contig_lines(VCF), report=("GP",))
    want = host.add_block(units, plain, ploidy_of, inbreeding_of, backend=Calling64)
    assert sorted(got) == sorted(want) and len(want) >= 3
    worst = 0.0
    for key in want:
        assert got[key] is not None and want[key] is not None
        H = len(units[key[0]]["locus"].haplotypes)
        ok, err = ref.within(got[key], want[key], comb(H + 3, 4))
        worst = max(worst, err)
        assert ok, (key, err)
    print("%s, block_path %s: %d units, worst |device - definition| %.3g" % (prior, block_path, len(want), worst))
    # the text: every non-numeric field equal, the numbers those of the definition up to their last written digit
    assert len(dev.lines) == len(host.lines)
    for a, b in zip(dev.lines, host.lines):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:7] == fb[:7] and fa[8] == fb[8] == "GT:GQ:PQ:DP:DS:GP"
        ia, ib = (dict(kv.split("=", 1) for kv in f[7].split(";")) for f in (fa, fb))
        assert {k: v for k, v in ia.items() if k != "ACP"} == {k: v for k, v in ib.items() if k != "ACP"}
        np.testing.assert_allclose(_numbers(ia["ACP"]), _numbers(ib["ACP"]), rtol=0, atol=0.0011)
        for ca, cb in zip(fa[9:], fb[9:]):
            ca, cb = ca.split(":"), cb.split(":")
            assert [ca[0], ca[2], ca[3]] == [cb[0], cb[2], cb[3]] and (ca[1] == ".") == (cb[1] == ".")
            if ca[1] != ".":
                assert abs(int(ca[1]) - int(cb[1])) <= 1
            np.testing.assert_allclose(_numbers(ca[4]), _numbers(cb[4]), rtol=0, atol=0.0011)
            np.testing.assert_allclose(_numbers(ca[5]), _numbers(cb[5]), rtol=0, atol=0.0011)


def test_one_record_per_block_and_the_plain_file(source):
    kw = dict(ploidy=4, inbreeding=0.1, prior_frequencies_tag="AFP")
    plain = list(application.call_exact(VCF, source, **kw))
    whole = application.SnvCalls(SAMPLES)
    each = application.SnvCalls(SAMPLES)
    assert list(application.call_exact(VCF, source, snv_calls=whole, **kw)) == plain
    assert list(application.call_exact(VCF, source, snv_calls=each, records_per_block=1, **kw)) == plain
    assert each.lines == whole.lines and all(ln.split("\t")[8] == "GT:GQ:PQ:DP:DS" for ln in whole.lines)
