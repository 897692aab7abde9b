"""GPU: the block path with base qualities in use and with pooled samples (block_path="wide").  call_reads_quals_kernel against the
host encoder, bit for bit; the exact caller and the call sampler fed the device-formed tensors against the same fed host tensors;
DenovoRaggedBatch.from_calls with qualities against the same units as float tensors; and the three programs' record lines with
block_path="wide" against the per-record / per-locus path, string for string."""
import io as _io
import os

import numpy as np
import pytest

from mchap_amd import application, blockpath, encoding, synth
from tests.call_blockpath_jobs import DEEP, HERE, SAMPLES, SHALLOW, haplotype_vcf, reference_bams

pytestmark = pytest.mark.gpu
ERR = 0.0024


def _compact(rows_calls, rows_quals, counts_of):
    """Compact arrays of units given as lists of int8 / int16 [rows_u, M] arrays: (calls, quals, counts, rows, call offsets,
    count offsets), the order device.call_reads_from_calls_quals takes."""
    rows = np.array([len(c) for c in rows_calls], dtype=np.int64)
    M = rows_calls[0].shape[1]
    calls = np.concatenate([c.reshape(-1) for c in rows_calls]).astype(np.int8)
    quals = np.concatenate([q.reshape(-1) for q in rows_quals]).astype(np.int16)
    counts = np.concatenate(counts_of).astype(np.int64)
    return calls, quals, counts, rows, np.cumsum(rows * M) - rows * M, np.cumsum(rows) - rows


def _host_encoder(rows_calls, rows_quals, counts_of, nal, R, A, error_rate):
    """encoding.encode_read_distributions of every unit with its qualities, padded the way the programs pad a shape group."""
    U, M = nal.shape
    reads = np.full((U, R, M, A), np.nan)
    counts = np.zeros((U, R), dtype=np.int64)
    for u, (c, q) in enumerate(zip(rows_calls, rows_quals)):
        if len(c):
            d = encoding.encode_read_distributions(nal[u].tolist(), c, q, error_rate=error_rate)
            reads[u, : len(c), :, : d.shape[2]] = d
            reads[u, : len(c), :, d.shape[2]:] = 0.0   # (a unit whose own alleles are fewer than the group's A)
            counts[u, : len(c)] = counts_of[u]
    return reads, counts


def _kernel_case(name):
    rng = np.random.default_rng(11)
    if name == "smallest":
        # padding rows, an empty unit, zero after NaN, an A that is no power of two; the qualities 0 (probability 0), 156 / 157 (one
        # table value), 163 (exactly 1 - error rate), the table's last index (200) and a gap cell with a quality
        nal = np.tile(np.array([2, 3, 2], dtype=np.int8), (3, 1))
        rows_calls = [np.zeros((0, 3), np.int8), np.array([[1, -1, 0]], np.int8),
                      np.array([[0, 2, 1], [-1, -1, -1], [1, 0, -1], [0, 1, 0], [1, 2, 1]], np.int8)]
        rows_quals = [np.zeros((0, 3), np.int16), np.array([[0, 77, 156]], np.int16),
                      np.array([[157, 163, 30], [1, 2, 3], [200, 41, 250], [156, 157, 0], [20, 20, 82]], np.int16)]
        return rows_calls, rows_quals, [np.zeros(0, int), np.array([7]), np.array([1, 2, 3, 4, 1 << 40])], nal, 5, 3
    if name == "grid":
        U, R, M, A = 70, 37, 5, 4   # 51 800 doubles: no multiple of the workgroup, several passes of a capped grid
        nal = rng.integers(2, A + 1, size=(U, M)).astype(np.int8)
        nal[0] = A
        rows_calls, rows_quals, counts_of = [], [], []
        for u in range(U):
            n = R if u == 3 else int(rng.integers(0, R + 1))
            rows_calls.append(rng.integers(-1, nal[u][None, :].repeat(n, axis=0)).astype(np.int8) if n else np.zeros((0, M), dtype=np.int8))
            q = rng.integers(0, 94, size=(n, M))
            rows_quals.append(np.where(rng.random((n, M)) < 0.1, rng.integers(150, 201, size=(n, M)), q).astype(np.int16))
            counts_of.append(rng.integers(1, 1000, size=n))
        return rows_calls, rows_quals, counts_of, nal, R, A
    assert name == "single"
    nal = np.full((2, 1), 2, dtype=np.int8)
    return [np.array([[1]], np.int8), np.array([[-1]], np.int8)], [np.array([[33]], np.int16), np.array([[60]], np.int16)], \
        [np.array([3]), np.array([4])], nal, 1, 2


@pytest.mark.parametrize("wide", [False, True], ids=["index32", "index64"])
@pytest.mark.parametrize("name", ["smallest", "grid", "single"])
def test_kernel_equals_the_host_encoder(name, wide, monkeypatch):
    """wide: the instantiation that divides the cell index in 64 bits (forced by MCHAP_HIP_CALL_READS_WIDE)."""
    if wide:
        monkeypatch.setenv("MCHAP_HIP_CALL_READS_WIDE", "1")
    else:
        monkeypatch.delenv("MCHAP_HIP_CALL_READS_WIDE", raising=False)
    from mchap_amd.device import call_reads_from_calls_quals

    rows_calls, rows_quals, counts_of, nal, R, A = _kernel_case(name)
    want_reads, want_counts = _host_encoder(rows_calls, rows_quals, counts_of, nal, R, A, ERR)
    calls, quals, counts, rows, c_off, n_off = _compact(rows_calls, rows_quals, counts_of)
    d_reads, d_counts = call_reads_from_calls_quals(calls, quals, counts, rows, c_off, n_off, nal, R, A, error_rate=ERR)
    got_reads, got_counts = d_reads.cpu().numpy(), d_counts.cpu().numpy()
    assert got_reads.shape == want_reads.shape and got_reads.dtype == np.float64 and got_counts.dtype == np.int64
    assert np.array_equal(got_reads, want_reads, equal_nan=True)
    assert np.array_equal(got_counts, want_counts)
    # where it is not NaN the tensor is the host's bit for bit
    assert np.array_equal(got_reads.view(np.uint64)[~np.isnan(want_reads)], want_reads.view(np.uint64)[~np.isnan(want_reads)])
    # ... and the host statement of the rule says the same
    ex_reads, ex_counts = blockpath.expand_call_units(calls, counts, rows, c_off, n_off, nal, R, A, error_rate=ERR, quals=quals)
    assert np.array_equal(ex_reads.view(np.uint64)[~np.isnan(want_reads)], want_reads.view(np.uint64)[~np.isnan(want_reads)])
    assert np.array_equal(np.isnan(ex_reads), np.isnan(want_reads)) and np.array_equal(ex_counts, want_counts)
    if name == "smallest":   # (the cases the table is about are there)
        called = quals[calls >= 0]
        assert {0, 156, 157, 163}.issubset(called.tolist()) and called.max() == 200 and quals[calls < 0].max() > 200


def test_kernel_units_in_any_order_of_the_compact_arrays():
    """The offsets, not the order, place a unit: units stored back to front, with unused elements between them (whose calls and
    qualities are never looked at); rows outside the arrays or a quality outside the table are refused on the host."""
    from mchap_amd.device import call_reads_from_calls_quals

    rows_calls, rows_quals, counts_of, nal, R, A = _kernel_case("smallest")
    want_reads, want_counts = _host_encoder(rows_calls, rows_quals, counts_of, nal, R, A, ERR)
    calls = np.full(64, 1, dtype=np.int8)
    quals = np.full(64, -9, dtype=np.int16)    # (unused elements: called, with a quality no table has)
    counts = np.full(32, -5, dtype=np.int64)
    calls[40:55], quals[40:55], counts[20:25] = rows_calls[2].reshape(-1), rows_quals[2].reshape(-1), counts_of[2]
    calls[7:10], quals[7:10], counts[3:4] = rows_calls[1].reshape(-1), rows_quals[1].reshape(-1), counts_of[1]
    d_reads, d_counts = call_reads_from_calls_quals(calls, quals, counts, [0, 1, 5], [0, 7, 40], [0, 3, 20], nal, R, A, error_rate=ERR)
    got = d_reads.cpu().numpy()
    assert np.array_equal(got, want_reads, equal_nan=True) and np.array_equal(d_counts.cpu().numpy(), want_counts)
    assert np.array_equal(got.view(np.uint64)[~np.isnan(want_reads)], want_reads.view(np.uint64)[~np.isnan(want_reads)])
    # a table longer than the qualities need: the same tensor
    d_reads, _ = call_reads_from_calls_quals(calls, quals, counts, [0, 1, 5], [0, 7, 40], [0, 3, 20], nal, R, A, error_rate=ERR, n_qual=300)
    assert np.array_equal(d_reads.cpu().numpy(), want_reads, equal_nan=True)
    with pytest.raises(AssertionError):
        call_reads_from_calls_quals(calls, quals, counts, [0, 1, 5], [0, 7, 50], [0, 3, 20], nal, R, A)   # (rows beyond the calls)
    with pytest.raises(AssertionError):
        call_reads_from_calls_quals(calls, quals, counts, [0, 1, 6], [0, 7, 40], [0, 3, 20], nal, R, A)   # (more rows than n_reads)
    with pytest.raises(AssertionError):
        call_reads_from_calls_quals(calls, quals, counts, [0, 1, 5], [0, 7, 40], [0, 3, 20], nal, R, A, n_qual=200)   # (a called cell of quality 200)
    with pytest.raises(AssertionError):
        call_reads_from_calls_quals(calls, quals, counts, [0, 1, 5], [0, 6, 40], [0, 3, 20], nal, R, A)   # (element 6: called, quality -9)
    with pytest.raises(AssertionError):
        call_reads_from_calls_quals(calls, quals[:-1], counts, [0, 1, 5], [0, 7, 40], [0, 3, 20], nal, R, A)   # (fewer qualities than calls)


def _small_group(seed=3, U=9, R=12, M=4, A=3, H=5):
    rng = np.random.default_rng(seed)
    nal = np.tile(np.array([2, 3, 2, 3], dtype=np.int8)[:M], (U, 1))
    haps = np.stack([np.stack([rng.integers(0, nal[0]) for _ in range(H)]) for _ in range(U)]).astype(np.int8)
    rows_calls, rows_quals, counts_of = [], [], []
    for u in range(U):
        n = 0 if u == 1 else int(rng.integers(1, R + 1))
        truth = haps[u][rng.integers(0, H, size=n)]
        rows_calls.append(np.where(rng.random((n, M)) < 0.15, -1, truth).astype(np.int8).reshape(n, M))
        rows_quals.append(rng.choice(np.array([3, 12, 20, 30, 41, 82, 157], dtype=np.int16), size=(n, M)))
        counts_of.append(rng.integers(1, 6, size=n))
    return rows_calls, rows_quals, counts_of, nal, haps, R, A


def _both_tensors(rows_calls, rows_quals, counts_of, nal, R, A):
    from mchap_amd.device import call_reads_from_calls_quals

    reads, counts = _host_encoder(rows_calls, rows_quals, counts_of, nal, R, A, ERR)
    return (reads, counts), call_reads_from_calls_quals(*_compact(rows_calls, rows_quals, counts_of), nal, R, A, error_rate=ERR)


@pytest.mark.parametrize("prior", [False, True])
def test_exact_batch_fed_device_quality_tensors(prior):
    from mchap_amd.device import ExactDeviceBatch

    rows_calls, rows_quals, counts_of, nal, haps, R, A = _small_group()
    (reads, counts), (d_reads, d_counts) = _both_tensors(rows_calls, rows_quals, counts_of, nal, R, A)
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
def test_call_sampler_fed_device_quality_tensors(prior):
    import dataclasses

    from mchap_amd.calling_mcmc import CallingMCMC
    from mchap_amd.device import CompactCallReads

    rows_calls, rows_quals, counts_of, nal, haps, R, A = _small_group(seed=4)
    (reads, counts), on_device = _both_tensors(rows_calls, rows_quals, counts_of, nal, R, A)
    U, H = haps.shape[:2]
    rng = np.random.default_rng(6)
    pr = (np.full(U, 0.1), rng.dirichlet(np.ones(H), size=U)) if prior else None
    model = CallingMCMC(ploidy=4, haplotypes=haps[0], steps=200, chains=2, random_seed=11)
    kw = dict(haplotypes=haps, prior=pr, stream_ids=np.zeros(U, dtype=np.uint64), burn=100)
    want = model.finish_batch_summaries(model.start_batch_summaries(reads, counts, **kw))
    got = model.finish_batch_summaries(model.start_batch_summaries(None, None, device_reads=on_device, **kw))
    # ... and given the compact form itself (what application.call passes): formed on the device inside the call
    calls, quals, cnts, rows, c_off, n_off = _compact(rows_calls, rows_quals, counts_of)
    compact = CompactCallReads(calls, cnts, rows, c_off, n_off, nal, R, A, error_rate=ERR, quals=quals)
    assert compact.shape == reads.shape and len(compact) == U and compact.counts.shape == counts.shape
    also = model.finish_batch_summaries(model.start_batch_summaries(compact, compact.counts, **kw))
    assert compact._host is None   # (nobody asked for the host tensor)
    assert len(want) == len(got) == len(also) == U
    for x, y, z in zip(want, got, also):
        for f in dataclasses.fields(x):
            assert np.array_equal(getattr(x, f.name), getattr(y, f.name)), f.name
            assert np.array_equal(getattr(x, f.name), getattr(z, f.name)), f.name
    # asked for on the host, the same tensor and counts
    assert np.array_equal(np.asarray(compact), reads, equal_nan=True) and np.array_equal(np.asarray(compact.counts), counts)


def test_from_calls_with_qualities_equals_the_tensor_batch():
    import torch

    from mchap_amd import DenovoMCMC
    from mchap_amd.device import DenovoRaggedBatch

    rng = np.random.default_rng(12)
    units, calls, quals, counts = [], [], [], []
    shapes = [(4, 7, 2, 30), (4, 3, 3, 12), (4, 12, 2, 1), (4, 1, 4, 25), (4, 9, 2, 60), (4, 5, 2, 1)]
    nal_flat, nal_off, r_off, c_off = [], [], [], []
    for i, (K, M, A, R) in enumerate(shapes):
        n_alleles = rng.integers(2, A + 1, size=M) if A > 2 else np.full(M, 2)
        haps = rng.integers(0, n_alleles, size=(K, M))
        c = haps[rng.integers(0, K, size=R)].astype(np.int8)
        c[rng.random(c.shape) < 0.2] = -1
        q = rng.choice(np.array([2, 15, 20, 30, 41, 82, 156, 157, 200], dtype=np.int16), size=c.shape)
        no_reads = R == 1 and i == 5
        if no_reads:
            c[:], q[:] = -1, 0          # a unit without reads: one all-gap row, no counts
        d = encoding.encode_read_distributions(n_alleles, c, q, error_rate=ERR)
        ud, cn = encoding.unique_counts(d)
        # the same distinct rows as calls and qualities: the first row of every group
        first = [int(np.flatnonzero([x.tobytes() == y.tobytes() for x in d])[0]) for y in ud]
        units.append(dict(reads=ud, counts=None if no_reads else cn, n_alleles=n_alleles, ploidy=K, inbreeding=0.1 * (i % 3) if i % 4 else None,
                          stream_id=0, temps=(1.0,)))
        r_off.append(sum(len(x) for x in calls))
        calls.append(c[first].reshape(-1))
        quals.append(q[first].reshape(-1))
        c_off.append(-1 if no_reads else sum(len(x) for x in counts))
        if not no_reads:
            counts.append(cn)
        nal_off.append(len(nal_flat))
        nal_flat += n_alleles.tolist()
    model = DenovoMCMC(ploidy=4, n_alleles=[2], steps=300, chains=2, random_seed=5)
    a = DenovoRaggedBatch(model, units)
    a.run(100)
    U = len(units)
    args = (model, np.concatenate(calls), np.array(r_off), np.array([len(u["reads"]) for u in units]), np.array([u["reads"].shape[1] for u in units]),
            np.array([u["reads"].shape[2] for u in units]), np.full(U, 4), np.concatenate(counts), np.array(c_off), np.array(nal_flat, dtype=np.int8),
            np.array(nal_off))
    kw = dict(inbreeding=np.array([np.nan if u["inbreeding"] is None else u["inbreeding"] for u in units]), error_rate=ERR)
    b = DenovoRaggedBatch.from_calls(*args, quals=np.concatenate(quals), **kw)
    b.run(100)
    torch.cuda.synchronize()
    assert torch.equal(a.d_trace, b.d_trace) and torch.equal(a.d_fixed, b.d_fixed) and torch.equal(a.d_status, b.d_status)
    assert np.array_equal(a.d_llks.cpu().numpy().view(np.uint64), b.d_llks.cpu().numpy().view(np.uint64))
    # (the qualities matter: without them the likelihoods are others)
    c_ = DenovoRaggedBatch.from_calls(*args, **kw)
    c_.run(100)
    torch.cuda.synchronize()
    assert not np.array_equal(a.d_llks.cpu().numpy(), c_.d_llks.cpu().numpy())
    bad = np.concatenate(quals)
    bad[np.flatnonzero(np.concatenate(calls) >= 0)[0]] = -1
    with pytest.raises(AssertionError):
        DenovoRaggedBatch.from_calls(*args, quals=bad, **kw)


# ---- the programs: record lines with block_path="wide" and record by record / locus by locus ----
def _counters(monkeypatch):
    """Counts of what formed the device input: {"quals": ..., "plain": ...} calls of device.call_reads_from_calls_quals /
    call_reads_from_calls, and of DenovoRaggedBatch.from_calls with / without qualities."""
    from mchap_amd import device

    n = dict(quals=0, plain=0)

    def counting(inner, key):
        def f(*a, **k):
            n[key] += 1
            return inner(*a, **k)
        return f
    monkeypatch.setattr(device, "call_reads_from_calls_quals", counting(device.call_reads_from_calls_quals, "quals"))
    monkeypatch.setattr(device, "call_reads_from_calls", counting(device.call_reads_from_calls, "plain"))
    inner = device.DenovoRaggedBatch.from_calls.__func__

    def from_calls(cls, *a, quals=None, **k):
        n["quals" if quals is not None else "plain"] += 1
        return inner(cls, *a, quals=quals, **k)
    monkeypatch.setattr(device.DenovoRaggedBatch, "from_calls", classmethod(from_calls))
    return n


class _Spy:
    """Counts the calls of a source's per-record reads()."""

    def __init__(self, source):
        self.n = 0
        inner = source.reads

        def reads(locus, sample):
            self.n += 1
            return inner(locus, sample)
        source.reads = reads


def _lines_both_ways(program, source, monkeypatch, run):
    """run(block_path) -> the program's lines.  The wide path must have formed its device input from the compact arrays (with
    qualities exactly when the source uses them) without a single per-record read: a silent fallback cannot pass."""
    n = _counters(monkeypatch)
    spy = _Spy(source)
    slow = run(False)
    assert n == dict(quals=0, plain=0) and spy.n > 0
    spy.n = 0
    fast = run("wide")
    assert spy.n == 0 and len(fast) > 0
    assert (n["quals"] > 0 and n["plain"] == 0) if source.use_phred else (n["plain"] > 0 and n["quals"] == 0)
    assert fast == slow
    return fast


def _pools(paths, names, which):
    a, b, c = [(s, paths[s]) for s in names]
    return {"POOL": [a, b, c]} if which == "one" else {"P1": [a, b], "P2": [c, a]}


def _reference_source(kind, files):
    paths = reference_bams(files)
    if kind == "phred":
        return application.ReadSource(paths, use_phred=True)
    # pooled both ways: one pool of all three with base qualities in use, two pools that share a file without
    return application.ReadSource(_pools(paths, SAMPLES, "one" if kind == "pool_one" else "two"), use_phred=kind == "pool_one")


def _run_program(program, source, vcf=None, assemble_kw=None, **kw):
    if program == "assemble":
        return lambda bp: list(application.assemble(sample_bams=source, block_path=bp, steps=400, burn=200, chains=2, seed=11, **assemble_kw, **kw))
    fn = getattr(application, program)
    if program == "call":
        kw = dict(dict(steps=200, burn=100), **kw)
    return lambda bp: list(fn(vcf, source, block_path=bp, **kw))


@pytest.mark.parametrize("program", ["call_exact", "call", "assemble"])
@pytest.mark.parametrize("kind", ["phred", "pool_one", "pool_two"])
@pytest.mark.parametrize("files", [SHALLOW, DEEP], ids=["simple", "deep"])
def test_reference_lines(program, kind, files, monkeypatch):
    from test_gpu_assemble_goldens import SEQ

    source = _reference_source(kind, files)
    ploidy = {s: (4 if i % 2 == 0 else 2) for i, s in enumerate(source.samples)}
    assemble_kw = dict(bed_path=os.path.join(HERE, "simple.bed"), variants_vcf_path=os.path.join(HERE, "simple.vcf"),
                       reference_sequences={c: SEQ for c in ("CHR1", "CHR2", "CHR3")})
    run = _run_program(program, source, os.path.join(HERE, "simple.output.assemble.vcf"), assemble_kw, ploidy=ploidy,
                       report=("GL",) if files is DEEP else ())
    _lines_both_ways(program, source, monkeypatch, run)


@pytest.fixture(scope="module")
def synth_job(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wide_block_gpu"))
    job = synth.synth_assembly_inputs(d, n_loci=30, n_samples=3, reads_per_locus=16, n_snvs=5, gap=30)
    job["haps"] = haplotype_vcf(job, os.path.join(d, "haps.vcf"), specials=True)
    job["pools"] = _pools(dict(zip(["S000", "S001", "S002"], job["bams"])), ["S000", "S001", "S002"], "two")
    return job


@pytest.mark.parametrize("program", ["call_exact", "call", "assemble"])
def test_pooled_synthetic_lines_with_base_qualities_in_several_blocks(program, synth_job, monkeypatch):
    """30 loci x 3 samples in two pools that share a file, base qualities in use, several blocks."""
    from mchap_amd import io

    source = application.ReadSource(synth_job["pools"], use_phred=True)
    assemble_kw = dict(bed_path=synth_job["bed"], variants_vcf_path=synth_job["vcf"], reference_sequences=io.Reference(synth_job["fasta"]),
                       units_per_block=2 * 8)
    extra = dict() if program == "assemble" else dict(records_per_block=7, inbreeding=0.1, prior_frequencies_tag="AFP")
    run = _run_program(program, source, synth_job["haps"], assemble_kw, ploidy={"P1": 4, "P2": 2}, **extra)
    lines = _lines_both_ways(program, source, monkeypatch, run)
    assert len(lines) == 30
    whole = _run_program(program, source, synth_job["haps"], dict(assemble_kw, units_per_block=None), ploidy={"P1": 4, "P2": 2},
                         **(dict(extra, records_per_block=4096) if extra else {}))("wide")
    assert whole == lines


def test_command_line_wide_equals_off(tmp_path):
    from mchap_amd import cli

    argv = ["mchap_amd", "call-exact", "--haplotypes", os.path.join(HERE, "simple.output.assemble.vcf"), "--ploidy", "4", "--use-base-phred-scores",
            "--bam"] + [os.path.join(HERE, f) for f in DEEP]
    out = {}
    for mode in ("off", "wide"):
        buf = _io.StringIO()
        n = cli.run(argv + ["--block-path", mode], out=buf)
        out[mode] = [ln for ln in buf.getvalue().splitlines() if not ln.startswith("##commandline")]
        assert n > 0 and len(out[mode]) > n
    assert out["off"] == out["wide"]
