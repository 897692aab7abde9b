"""call-exact --allele-depths on the device, end to end on the reference's files (tetraploid, three samples): the arrays
AlleleDepths.add_block returns against the definition (application.allele_support_host) on the library's own float64 likelihoods,
the file's text against the definition's, and the record lines with and without the writer -- under the flat prior, the
Dirichlet-multinomial prior and after the frequency estimate, record by record and on the block path."""
import os

import numpy as np
import pytest

from mchap_amd import application
from tests import allele_support_reference as ref
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
    depths = application.AlleleDepths(SAMPLES)
    assert list(application.call_exact(VCF, source, allele_depths=depths, **kw)) == plain      # the record lines are identical
    assert len(depths.lines) == len(plain) >= 3
    # the same block by hand: the device's arrays against the definition on the library's float64 likelihoods
    _, records = application.read_vcf(VCF)
    tag = PRIORS[prior].get("prior_frequencies_tag")
    units = application._exact_units(records, source, SAMPLES, tag, None, block_path)
    ploidy_of, inbreeding_of = (lambda s: 4), (lambda s: PRIORS[prior].get("inbreeding"))
    if prior == "estimate":
        application.estimate_prior_frequencies(units, SAMPLES, ploidy_of, inbreeding_of, 5)
    dev = application.AlleleDepths(SAMPLES)
    got = dev.add_block(units, plain, ploidy_of, inbreeding_of)
    assert dev.lines == depths.lines                                                          # the program's file is this file
    host = application.AlleleDepths(SAMPLES)
    want = host.add_block(units, plain, ploidy_of, inbreeding_of, backend=Calling64)
    assert sorted(got) == sorted(want) and len(want) >= 3
    worst = 0.0
    for key in want:
        assert got[key] is not None and want[key] is not None
        N = float(np.sum(units[key[0]]["reads"][key[1]]["counts"]))
        ok, err = ref.within(got[key], want[key], N)
        worst = max(worst, err)
        assert ok, (key, err)
        assert abs(got[key].sum() - N) <= len(got[key]) * (ref.REL * N + ref.floor(N))
    print("%s, block_path %s: %d units, worst |device - definition| %.3g" % (prior, block_path, len(want), worst))
    # the text: every other field equal, the numbers those of the definition up to their last written digit
    assert len(dev.lines) == len(host.lines)
    for a, b, p in zip(dev.lines, host.lines, plain):
        fa, fb, fp = a.split("\t"), b.split("\t"), p.split("\t")
        assert fa[:7] == fb[:7] == fp[:7] and fa[8] == fb[8] == fp[8] + ":ADP"
        assert fa[7].rsplit(";ADP=", 1)[0] == fb[7].rsplit(";ADP=", 1)[0] == fp[7]
        np.testing.assert_allclose(_numbers(fa[7].rsplit(";ADP=", 1)[1]), _numbers(fb[7].rsplit(";ADP=", 1)[1]), rtol=0, atol=0.0011)
        for ca, cb, cp in zip(fa[9:], fb[9:], fp[9:]):
            assert ca.rsplit(":", 1)[0] == cb.rsplit(":", 1)[0] == cp
            np.testing.assert_allclose(_numbers(ca.rsplit(":", 1)[1]), _numbers(cb.rsplit(":", 1)[1]), rtol=0, atol=0.0011)


def test_one_record_per_block(source):
    kw = dict(ploidy=4, inbreeding=0.1, prior_frequencies_tag="AFP")
    plain = list(application.call_exact(VCF, source, **kw))
    whole = application.AlleleDepths(SAMPLES)
    each = application.AlleleDepths(SAMPLES)
    assert list(application.call_exact(VCF, source, allele_depths=whole, **kw)) == plain
    assert list(application.call_exact(VCF, source, allele_depths=each, records_per_block=1, **kw)) == plain
    # (a unit's reads are padded to its chunk's deepest unit, and the likelihood adds the rows four to a logarithm: the blocks'
    # likelihoods differ in their last bits, the written depths in no digit but a rounding's)
    for a, b in zip(each.lines, whole.lines):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:7] == fb[:7] and fa[8] == fb[8]
        for ca, cb in zip([fa[7].rsplit(";ADP=", 1)[1]] + [c.rsplit(":", 1)[1] for c in fa[9:]],
                          [fb[7].rsplit(";ADP=", 1)[1]] + [c.rsplit(":", 1)[1] for c in fb[9:]]):
            np.testing.assert_allclose(_numbers(ca), _numbers(cb), rtol=0, atol=0.0011)
