"""GPU: the block path of `mchap call` / `mchap call-exact`.  call_reads_kernel against the host encoder, bit for bit; the exact
caller and the call sampler fed device tensors against the same fed host tensors; and the programs' record lines with the block
path against the per-record path (and the default), string for string."""
import os

import numpy as np
import pytest

from mchap_amd import application, encoding, synth
from tests.call_blockpath_jobs import HERE, MIXED, REFERENCE_JOBS, haplotype_vcf, reference_bams

pytestmark = pytest.mark.gpu
ERR = 0.0024


def _compact(rows_calls, counts_of):
    """Compact arrays of units given as lists of int8 [rows_u, M] arrays."""
    rows = np.array([len(c) for c in rows_calls], dtype=np.int64)
    M = rows_calls[0].shape[1]
    calls = np.concatenate([c.reshape(-1) for c in rows_calls]).astype(np.int8)
    counts = np.concatenate(counts_of).astype(np.int64)
    return calls, counts, rows, np.cumsum(rows * M) - rows * M, np.cumsum(rows) - rows


def _host_encoder(rows_calls, counts_of, nal, R, A, error_rate):
    """encoding.encode_read_distributions of every unit, padded the way the programs pad a shape group."""
    U, M = nal.shape
    reads = np.full((U, R, M, A), np.nan)
    counts = np.zeros((U, R), dtype=np.int64)
    for u, c in enumerate(rows_calls):
        if len(c):
            d = encoding.encode_read_distributions(nal[u].tolist(), c, None, error_rate=error_rate)
            reads[u, : len(c), :, : d.shape[2]] = d
            reads[u, : len(c), :, d.shape[2]:] = 0.0   # (a unit whose own alleles are fewer than the group's A)
            counts[u, : len(c)] = counts_of[u]
    return reads, counts


def _random_units(rng, U, R, M, A, nal):
    rows_calls, counts_of = [], []
    for u in range(U):
        n = int(rng.integers(0, R + 1))
        c = rng.integers(-1, nal[u][None, :].repeat(n, axis=0)).astype(np.int8) if n else np.zeros((0, M), dtype=np.int8)
        rows_calls.append(c)
        counts_of.append(rng.integers(1, 1000, size=n))
    return rows_calls, counts_of


def _kernel_case(name):
    rng = np.random.default_rng(11)
    if name == "smallest":
        # padding rows, an empty unit, zero after NaN, an A that is no power of two; gaps and a call of the last allele
        nal = np.tile(np.array([2, 3, 2], dtype=np.int8), (3, 1))
        rows_calls = [np.zeros((0, 3), np.int8), np.array([[1, -1, 0]], np.int8),
                      np.array([[0, 2, 1], [-1, -1, -1], [1, 0, -1], [0, 1, 0], [1, 2, 1]], np.int8)]
        return rows_calls, [np.zeros(0, int), np.array([7]), np.array([1, 2, 3, 4, 1 << 40])], nal, 5, 3
    if name == "grid":
        U, R, M, A = 70, 37, 5, 4   # 51 800 doubles: no multiple of the workgroup, several passes of a capped grid
        nal = rng.integers(2, A + 1, size=(U, M)).astype(np.int8)
        nal[0] = A
        rows_calls, counts_of = _random_units(rng, U, R, M, A, nal)
        rows_calls[3], counts_of[3] = rng.integers(-1, 2, size=(R, M)).astype(np.int8), rng.integers(1, 9, size=R)   # (a full unit)
        return rows_calls, counts_of, nal, R, A
    assert name == "single"
    nal = np.full((2, 1), 2, dtype=np.int8)
    return [np.array([[1]], np.int8), np.array([[-1]], np.int8)], [np.array([3]), np.array([4])], nal, 1, 2


@pytest.mark.parametrize("wide", [False, True], ids=["index32", "index64"])
@pytest.mark.parametrize("name", ["smallest", "grid", "single"])
def test_kernel_equals_the_host_encoder(name, wide, monkeypatch):
    """wide: the instantiation that divides the cell index in 64 bits (what more than 2^32 cells run; forced here by
    MCHAP_HIP_CALL_READS_WIDE, since a tensor of that size is 32 GiB)."""
    if wide:
        monkeypatch.setenv("MCHAP_HIP_CALL_READS_WIDE", "1")
    else:
        monkeypatch.delenv("MCHAP_HIP_CALL_READS_WIDE", raising=False)
    from mchap_amd import blockpath
    from mchap_amd.device import call_reads_from_calls

    rows_calls, counts_of, nal, R, A = _kernel_case(name)
    want_reads, want_counts = _host_encoder(rows_calls, counts_of, nal, R, A, ERR)
    calls, counts, rows, c_off, n_off = _compact(rows_calls, counts_of)
    d_reads, d_counts = call_reads_from_calls(calls, counts, rows, c_off, n_off, nal, R, A, error_rate=ERR)
    got_reads, got_counts = d_reads.cpu().numpy(), d_counts.cpu().numpy()
    assert got_reads.shape == want_reads.shape and got_reads.dtype == np.float64 and got_counts.dtype == np.int64
    assert np.array_equal(got_reads, want_reads, equal_nan=True)
    assert np.array_equal(got_counts, want_counts)
    # where it is not NaN the tensor is the host's bit for bit
    assert np.array_equal(got_reads.view(np.uint64)[~np.isnan(want_reads)], want_reads.view(np.uint64)[~np.isnan(want_reads)])
    # ... and the host statement of the rule says the same
    ex_reads, ex_counts = blockpath.expand_call_units(calls, counts, rows, c_off, n_off, nal, R, A, error_rate=ERR)
    assert np.array_equal(ex_reads, want_reads, equal_nan=True) and np.array_equal(ex_counts, want_counts)


def test_kernel_units_in_any_order_of_the_compact_arrays():
    """The offsets, not the order, place a unit: units stored back to front, with unused elements between them."""
    from mchap_amd.device import call_reads_from_calls

    rows_calls, counts_of, nal, R, A = _kernel_case("smallest")
    want_reads, want_counts = _host_encoder(rows_calls, counts_of, nal, R, A, ERR)
    calls = np.full(64, 1, dtype=np.int8)
    counts = np.full(32, -5, dtype=np.int64)
    calls[40:55], counts[20:25] = rows_calls[2].reshape(-1), counts_of[2]
    calls[7:10], counts[3:4] = rows_calls[1].reshape(-1), counts_of[1]
    d_reads, d_counts = call_reads_from_calls(calls, counts, [0, 1, 5], [0, 7, 40], [0, 3, 20], nal, R, A, error_rate=ERR)
    assert np.array_equal(d_reads.cpu().numpy(), want_reads, equal_nan=True) and np.array_equal(d_counts.cpu().numpy(), want_counts)
    with pytest.raises(AssertionError):
        call_reads_from_calls(calls, counts, [0, 1, 5], [0, 7, 50], [0, 3, 20], nal, R, A)   # (rows beyond the calls)
    with pytest.raises(AssertionError):
        call_reads_from_calls(calls, counts, [0, 1, 6], [0, 7, 40], [0, 3, 20], nal, R, A)   # (more rows than n_reads)


def _small_group(seed=3, U=9, R=12, M=4, A=3, H=5):
    rng = np.random.default_rng(seed)
    nal = np.tile(np.array([2, 3, 2, 3], dtype=np.int8)[:M], (U, 1))
    haps = np.stack([np.stack([rng.integers(0, nal[0]) for _ in range(H)]) for _ in range(U)]).astype(np.int8)
    rows_calls, counts_of = [], []
    for u in range(U):
        n = 0 if u == 1 else int(rng.integers(1, R + 1))
        truth = haps[u][rng.integers(0, H, size=n)]
        c = np.where(rng.random((n, M)) < 0.15, -1, truth).astype(np.int8).reshape(n, M)
        rows_calls.append(c)
        counts_of.append(rng.integers(1, 6, size=n))
    return rows_calls, counts_of, nal, haps, R, A


def _both_tensors(rows_calls, counts_of, nal, R, A):
    from mchap_amd.device import call_reads_from_calls

    reads, counts = _host_encoder(rows_calls, counts_of, nal, R, A, ERR)
    return (reads, counts), call_reads_from_calls(*_compact(rows_calls, counts_of), nal, R, A, error_rate=ERR)


@pytest.mark.parametrize("prior", [False, True])
def test_exact_batch_fed_device_tensors(prior):
    from mchap_amd.device import ExactDeviceBatch

    rows_calls, counts_of, nal, haps, R, A = _small_group()
    (reads, counts), (d_reads, d_counts) = _both_tensors(rows_calls, counts_of, nal, R, A)
    U, H = haps.shape[:2]
    rng = np.random.default_rng(5)
    pr = (np.full(U, 0.1), rng.dirichlet(np.ones(H), size=U)) if prior else None
    host = ExactDeviceBatch(reads, 4, haps, counts, pr)
    dev = ExactDeviceBatch.from_device_reads(d_reads, 4, haps, d_counts, pr)
    assert dev.shape == host.shape and dev.G == host.G
    for b in (host, dev):
        b.run(streaming=True, arrays=True)
    for x, y in zip(host.mode_results(), dev.mode_results()):
        assert np.array_equal(x, y, equal_nan=True)
    a, b = host.array_results(True), dev.array_results(True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("prior", [False, True])
def test_call_sampler_fed_device_tensors(prior):
    import dataclasses

    from mchap_amd.calling_mcmc import CallingMCMC
    from mchap_amd.device import CompactCallReads

    rows_calls, counts_of, nal, haps, R, A = _small_group(seed=4)
    (reads, counts), on_device = _both_tensors(rows_calls, counts_of, nal, R, A)
    U, H = haps.shape[:2]
    rng = np.random.default_rng(6)
    pr = (np.full(U, 0.1), rng.dirichlet(np.ones(H), size=U)) if prior else None
    model = CallingMCMC(ploidy=4, haplotypes=haps[0], steps=200, chains=2, random_seed=11)
    kw = dict(haplotypes=haps, prior=pr, stream_ids=np.zeros(U, dtype=np.uint64), burn=100)
    want = model.finish_batch_summaries(model.start_batch_summaries(reads, counts, **kw))
    got = model.finish_batch_summaries(model.start_batch_summaries(None, None, device_reads=on_device, **kw))
    # ... and given the compact form itself (what application.call passes): formed on the device inside the call
    compact = CompactCallReads(*_compact(rows_calls, counts_of), nal, R, A, error_rate=ERR)
    assert compact.shape == reads.shape and len(compact) == U and compact.counts.shape == counts.shape
    also = model.finish_batch_summaries(model.start_batch_summaries(compact, compact.counts, **kw))
    assert compact._host is None   # (nobody asked for the host tensor)
    assert len(want) == len(got) == len(also) == U
    for x, y, z in zip(want, got, also):
        for f in dataclasses.fields(x):
            assert np.array_equal(getattr(x, f.name), getattr(y, f.name)), f.name
            assert np.array_equal(getattr(x, f.name), getattr(z, f.name)), f.name
    # asked for on the host (a stand-in sampler, the host classes), the same tensor and counts
    assert np.array_equal(np.asarray(compact), reads, equal_nan=True) and np.array_equal(np.asarray(compact.counts), counts)
    assert np.array_equal(compact[2], reads[2], equal_nan=True)


# ---- the programs: record lines with the block path and record by record ----
@pytest.fixture(scope="module")
def synth_job(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("call_block_gpu"))
    job = synth.synth_assembly_inputs(d, n_loci=30, n_samples=3, reads_per_locus=16, n_snvs=5, gap=30)
    job["haps"] = haplotype_vcf(job, os.path.join(d, "haps.vcf"), specials=True)
    job["source"] = application.ReadSource(dict(zip(["S000", "S001", "S002"], job["bams"])))
    return job


@pytest.fixture(scope="module")
def reference_sources():
    return {tuple(files): application.ReadSource(reference_bams(files)) for files in {tuple(f) for _, f in REFERENCE_JOBS}}


def _lines_both_ways(program, vcf, source, monkeypatch, **kw):
    from mchap_amd import device

    n = [0]
    inner = device.call_reads_from_calls

    def counted(*a, **k):
        n[0] += 1
        return inner(*a, **k)
    monkeypatch.setattr(device, "call_reads_from_calls", counted)
    if program is application.call:
        kw = dict(dict(steps=200, burn=100), **kw)
    slow = list(program(vcf, source, block_path=False, **kw))
    assert n[0] == 0
    fast = list(program(vcf, source, block_path=True, **kw))
    assert n[0] > 0 and len(fast) > 0
    assert fast == slow
    # block_path=None where the block path is the default (application.CALL_BLOCK_PATH_DEFAULT): the block path, the same lines
    monkeypatch.setattr(application, "CALL_BLOCK_PATH_DEFAULT", True)
    before = n[0]
    assert list(program(vcf, source, **kw)) == slow and n[0] > before
    return fast, n[0]


EXACT_OPTIONS = {
    "flat": dict(),
    "prior": dict(inbreeding=0.1, prior_frequencies_tag="AFP", report=("AFPRIOR",)),
    "report": dict(report=("GP", "GL", "AFP")),
    "ploidy": dict(ploidy={"S000": 2, "S001": 4, "S002": 2}),
    "filter": dict(filter_input_haplotypes="AFP>=0.1", prior_frequencies_tag="AFP", inbreeding=0.1),
}


@pytest.mark.parametrize("program", ["call_exact", "call"])
@pytest.mark.parametrize("vcf,bams", REFERENCE_JOBS)
def test_reference_lines(program, vcf, bams, reference_sources, monkeypatch):
    _lines_both_ways(getattr(application, program), os.path.join(HERE, vcf), reference_sources[tuple(bams)], monkeypatch)


@pytest.mark.parametrize("program", ["call_exact", "call"])
def test_reference_lines_with_prior_report_and_filter(program, reference_sources, monkeypatch):
    vcf = os.path.join(HERE, "mock.input.frequencies.vcf")
    source = reference_sources[tuple(MIXED)]
    for kw in (dict(inbreeding=0.1, prior_frequencies_tag="AFP", report=("AFPRIOR", "AFP")), dict(report=("GP", "GL", "AFP")),
               dict(filter_input_haplotypes="AFP>=0.1", prior_frequencies_tag="AFP", inbreeding=0.1, report=("AFP",)),
               dict(ploidy={"SAMPLE1": 2, "SAMPLE2": 4, "SAMPLE3": 2})):
        _lines_both_ways(getattr(application, program), vcf, source, monkeypatch, **kw)


@pytest.mark.parametrize("program", ["call_exact", "call"])
@pytest.mark.parametrize("options", sorted(EXACT_OPTIONS))
def test_synthetic_lines(program, options, synth_job, monkeypatch):
    """30 loci x 3 samples; the list ends with a record without variable positions, a REFMASKED record and (under the prior
    tag) an AF0 record."""
    lines, _ = _lines_both_ways(getattr(application, program), synth_job["haps"], synth_job["source"], monkeypatch, **EXACT_OPTIONS[options])
    assert len(lines) == 30
    f = [ln.split("\t") for ln in lines[-3:]]
    assert "NVAR=0;" in f[0][7] and "REFMASKED" in f[1][7]
    if "prior_frequencies_tag" in EXACT_OPTIONS[options]:
        # (all prior frequencies zero: AF0 -- or, once the filter has removed every alternate and masked the reference, NOA)
        assert f[2][6] == ("NOA" if "filter_input_haplotypes" in EXACT_OPTIONS[options] else "AF0")


@pytest.mark.parametrize("program", ["call_exact", "call"])
def test_several_blocks_and_several_chunks(program, synth_job, monkeypatch):
    fn = getattr(application, program)
    whole, n_whole = _lines_both_ways(fn, synth_job["haps"], synth_job["source"], monkeypatch)
    blocks, n_blocks = _lines_both_ways(fn, synth_job["haps"], synth_job["source"], monkeypatch, records_per_block=7)
    assert blocks == whole and n_blocks > n_whole
    monkeypatch.setattr(application, "device_unit_budget", lambda *a, **k: 11)
    chunks, n_chunks = _lines_both_ways(fn, synth_job["haps"], synth_job["source"], monkeypatch)
    assert chunks == whole and n_chunks > n_whole
