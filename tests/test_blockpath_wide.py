"""The block path with base qualities in use and with pooled samples (block_path="wide") on the host side: blockpath.encode_block with
a quality table against the per-record encoder -- the distinct FLOAT rows, byte for byte, in the same order with the same counts,
which is what the reference de-duplicates on --, pooled piles, the host statement of the device rule, which sources the wide gate
takes and what the keyword and the command line do with it.  No GPU here: tests/test_gpu_blockpath_wide.py has the kernel and the
programs' lines."""
import os
import re

import numpy as np
import pytest

from mchap_amd import application, blockpath, cli, encoding, io, sources, synth
from tests.call_blockpath_jobs import HERE, REFERENCE_JOBS, SAMPLES, haplotype_vcf, reference_bams
from tests.test_blockpath import _as_dict, _fake_summary
from tests.test_call_blockpath import _Replay, _Spy

ERR = 0.0024
QUALS = np.array([0, 20, 30, 41, 82, 156, 157, 163, 200, 255], dtype=np.int16)


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_table_is_the_encoders_value_and_saturates():
    """Entry q of the table is what encode_read_distributions gives a called cell of quality q, whatever the array it sits in;
    different qualities share a value from q = 156 on (so rows that differ only there are one float row)."""
    table = blockpath.qual_prob_table(ERR, 511)
    assert table.dtype == np.float64 and table[0] == 0.0 and table[156] == table[157] and table[155] != table[156]
    assert (table[163:] == 1.0 - ERR).all()
    canon = blockpath.canonical_qualities(table)
    assert canon[157] == 156 and canon[155] == 155 and canon[0] == 0 and (canon <= np.arange(511)).all()
    assert (table[canon] == table).all()
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 7, 8, 9, 31, 64, 511, 1000):
        q = rng.integers(0, 511, size=(n, 1)).astype(np.int16)
        d = encoding.encode_read_distributions([2], np.zeros((n, 1), dtype=np.int8), q, error_rate=ERR)
        assert d[:, 0, 0].tobytes() == table[q[:, 0]].tobytes()
        assert d[:, 0, 1].tobytes() == ((1.0 - table[q[:, 0]]) / 3.0).tobytes()


# ---- encoding of random piles ----
def _random_locus(rng, name, M):
    pos = np.sort(rng.choice(np.arange(5, 95), size=M, replace=False))
    variants = []
    for p in pos:
        ref = str(rng.choice(list("ACGT")))
        alts = tuple(str(x) for x in rng.permutation([b for b in "ACGT" if b != ref])[: int(rng.integers(1, 4))])
        variants.append(dict(chrom="c", pos=int(p) + 1, id=".", ref=ref, alts=alts, info={}))
    return io.DenovoLocus("c", 0, 100, name, variants, "A" * 100)


def _random_matrices(rng, locus, n):
    M = len(locus.positions)
    chars = rng.choice(np.frombuffer(b"ACGT-N", dtype=np.uint8), size=(n, M), p=[0.2, 0.2, 0.2, 0.2, 0.15, 0.05])
    quals = rng.choice(QUALS, size=(n, M))
    if n >= 6:
        # rows that can only be one float row: copies that differ in the quality of a gap cell, or by 156 against 157 (one table
        # value) in a called cell -- and a copy that differs by 155 against 156, which is another row
        chars[1], quals[1] = chars[0], quals[0]
        chars[0, 0] = chars[1, 0] = ord("-")
        quals[0, 0], quals[1, 0] = 30, 82
        called = locus.alleles[M - 1][0]
        for r, q in ((2, 156), (3, 157), (4, 155)):
            chars[r], quals[r] = chars[5], quals[5]
            chars[r, M - 1], quals[r, M - 1] = ord(called), q
    return chars, quals


def _merged_pairs(calls, quals):
    """(pairs of rows that differ only in the quality of gap cells, pairs that differ only by 156 against 157 in called cells)."""
    gap = sat = 0
    for a in range(len(calls)):
        for b in range(a + 1, len(calls)):
            d = quals[a] != quals[b]
            if (calls[a] != calls[b]).any() or not d.any():
                continue
            if (calls[a][d] < 0).all():
                gap += 1
            elif (calls[a][d] >= 0).all() and all({int(x), int(y)} == {156, 157} for x, y in zip(quals[a][d], quals[b][d])):
                sat += 1
    return gap, sat


def _expansion(locus, d, table):
    """The float rows of a locus's distinct rows, by the host statement of the device rule."""
    n, M = d["ucalls"].shape
    nal = np.array([locus.n_alleles], dtype=np.int8)
    reads, counts = blockpath.expand_call_units(d["ucalls"].reshape(-1), d["counts"], [n], [0], [0], nal, max(n, 1), int(max(locus.n_alleles)),
                                                error_rate=ERR, quals=d["uquals"].reshape(-1), quality_table=table)
    assert counts[0, :n].tolist() == d["counts"].tolist()
    return reads[0, :n]


@pytest.mark.parametrize("M", [1, 3, 5])
def test_random_piles_encode_to_the_per_record_float_rows(M):
    rng = np.random.default_rng(40 + M)
    loci = [_random_locus(rng, "t%d" % i, M) for i in range(14)]
    sizes = [0, 1, 2, 6, 40, 17, 9, 40, 6, 0, 33, 25, 12, 7]
    matrices = [_random_matrices(rng, l, n) for l, n in zip(loci, sizes)]
    pile = blockpath.pile_from_matrices(loci, matrices)
    table = blockpath.qual_prob_table(ERR, 256)
    enc = blockpath.encode_block(loci, pile, quality_table=table)
    plain = blockpath.encode_block(loci, pile)
    assert plain.uquals is None and plain.per_locus(3)["uquals"] is None   # (without a table: as before)
    gap = sat = merged = 0
    for li, (locus, (chars, quals)) in enumerate(zip(loci, matrices)):
        want = sources.encode_reads(locus, chars, quals, ERR, use_phred=True)
        d = enc.per_locus(li)
        np.testing.assert_array_equal(want["calls"], d["calls"])
        assert d["uquals"].dtype == np.int16 and d["uquals"].shape == d["ucalls"].shape
        np.testing.assert_array_equal(want["counts"], d["counts"])
        assert want["dists"].shape == (len(d["counts"]), M, max(locus.n_alleles))
        got = application._block_dists(locus.n_alleles, d["ucalls"], d["uquals"], ERR, table)
        assert _same_bytes(got, want["dists"])
        if len(d["counts"]):
            assert _same_bytes(_expansion(locus, d, table), want["dists"])
        g, s_ = _merged_pairs(want["calls"], quals)
        gap, sat = gap + g, sat + s_
        merged += int((np.asarray(want["counts"]) > 1).sum())
        # without qualities the same pile has fewer (or as many) distinct rows
        assert len(plain.per_locus(li)["counts"]) <= len(d["counts"])
    assert gap > 0 and sat > 0 and merged > 0


def test_a_negative_quality_in_a_called_cell_is_left_to_the_per_record_path():
    rng = np.random.default_rng(3)
    locus = _random_locus(rng, "t", 3)
    chars = np.frombuffer((locus.alleles[0][0] + "-" + locus.alleles[2][1]).encode(), dtype=np.uint8).reshape(1, 3)
    table = blockpath.qual_prob_table(ERR, 64)
    ok = blockpath.pile_from_matrices([locus], [(chars, np.array([[30, -7, 40]]))])      # (negative in a gap: no matter)
    assert blockpath.encode_block([locus], ok, quality_table=table).ucounts.tolist() == [1]
    for bad in ([[-1, 0, 40]], [[30, 0, 64]]):                                             # (negative; beyond the table)
        with pytest.raises(blockpath.BlockPathUnavailable):
            blockpath.encode_block([locus], blockpath.pile_from_matrices([locus], [(chars, np.array(bad))]), quality_table=table)


# ---- the reference's files, pooled samples ----
def _units_both_ways(vcf, source, prior_tag=None):
    _, records = io.read_vcf(vcf)
    slow = application._exact_units(records, source, source.samples, prior_tag, None, False)
    fast = application._exact_units(records, source, source.samples, prior_tag, None, "wide")
    assert len(slow) == len(fast) == len(records)
    assert all(u["block"] is not None for u in fast) and all(u["block"] is None for u in slow)
    return slow, fast


def _same_inputs(slow, fast, samples, use_phred):
    """chars, calls, depth, the distinct float rows (byte for byte) in order of first appearance, their counts."""
    n = merged = 0
    for a, b in zip(slow, fast):
        assert a["invalid"] == b["invalid"] and a["needs_kernel"] == b["needs_kernel"]
        M = len(a["locus"].positions)
        for s in samples:
            x, y = a["reads"][s], b["reads"][s]
            np.testing.assert_array_equal(x["chars"], y["chars"])
            assert x["calls"].shape == y["calls"].shape and x["calls"].dtype == y["calls"].dtype
            np.testing.assert_array_equal(x["calls"], y["calls"])
            np.testing.assert_array_equal(np.asarray(x["depth"], dtype=np.int64), np.asarray(y["depth"], dtype=np.int64))
            np.testing.assert_array_equal(x["counts"], y["counts"])
            if M:
                assert (y["uquals"] is not None) == use_phred
                assert _same_bytes(x["dists"], y["dists"])
            n += len(x["calls"])
            merged += int((np.asarray(x["counts"]) > 1).sum())
    return n, merged


@pytest.mark.parametrize("vcf,bams", REFERENCE_JOBS)
def test_reference_records_with_base_qualities_encode_the_same(vcf, bams):
    source = application.ReadSource(reference_bams(bams), use_phred=True)
    slow, fast = _units_both_ways(os.path.join(HERE, vcf), source)
    n, _ = _same_inputs(slow, fast, SAMPLES, True)
    assert n > 50


def _pools(paths, which):
    a, b, c = [(s, paths[s]) for s in SAMPLES]
    return {"POOL": [a, b, c]} if which == "one" else {"P1": [a, b], "P2": [c, a]}


@pytest.mark.parametrize("use_phred", [False, True])
@pytest.mark.parametrize("which", ["one", "two"])
@pytest.mark.parametrize("vcf,bams", [REFERENCE_JOBS[0], REFERENCE_JOBS[3]])
def test_pooled_samples_encode_the_same(vcf, bams, which, use_phred, monkeypatch):
    source = application.ReadSource(_pools(reference_bams(bams), which), use_phred=use_phred)
    assert not sources._block_path_takes(source) and sources._block_path_takes(source, wide=True)
    extracted = []
    inner = blockpath.extract_block
    monkeypatch.setattr(blockpath, "extract_block", lambda loci, cols, sample, **kw: extracted.append(sample) or inner(loci, cols, sample, **kw))
    slow, fast = _units_both_ways(os.path.join(HERE, vcf), source)
    assert sorted(extracted) == SAMPLES   # (a (read group, file) pair two pools share is extracted once)
    n, merged = _same_inputs(slow, fast, source.samples, use_phred)
    assert n > 50 and (use_phred or merged > 0)
    # a pool's depth is the sum of its members'
    alone = application._exact_units([u["rec"] for u in slow], application.ReadSource(reference_bams(bams)), SAMPLES, None, None, False)
    members = {"POOL": SAMPLES, "P1": SAMPLES[:2], "P2": [SAMPLES[2], SAMPLES[0]]}
    for u, v in zip(fast, alone):
        for pool in source.samples:
            assert len(u["reads"][pool]["calls"]) == sum(len(v["reads"][s]["calls"]) for s in members[pool])


def test_concat_piles_is_the_row_wise_concatenation_locus_by_locus():
    rng = np.random.default_rng(9)
    loci = [_random_locus(rng, "a", 3), _random_locus(rng, "b", 1), io.DenovoLocus("c", 0, 100, "none", [], "A" * 100), _random_locus(rng, "d", 5)]
    groups = [[_random_matrices(rng, l, n) for l, n in zip(loci, ns)] for ns in ((4, 0, 2, 7), (0, 0, 0, 0), (3, 5, 1, 0))]
    piles = [blockpath.pile_from_matrices(loci, g) for g in groups]
    assert blockpath.concat_piles(piles[:1]) is piles[0]
    both = blockpath.concat_piles(piles)
    assert both.row_start.tolist() == [0, 7, 12, 15, 22] and both.chars.dtype == np.uint8 and both.quals.dtype == np.int16
    for li in range(4):
        chars, quals = both.matrices(li)
        np.testing.assert_array_equal(chars, np.concatenate([g[li][0] for g in groups]))
        np.testing.assert_array_equal(quals, np.concatenate([g[li][1] for g in groups]))
    np.testing.assert_array_equal(both.row_locus, np.repeat(np.arange(4), [7, 5, 3, 7]))
    np.testing.assert_array_equal(both.cell_of_row[both.row_start[:-1][[0, 1, 3]]], both.cell_start[:-1][[0, 1, 3]])


def test_expand_rule_small_case_with_qualities():
    """The rule of include/mchap_hip.h with base qualities spelled out: the small case of tests/test_call_blockpath.py with the
    qualities 0 (probability 0 for the called allele), 157 (the saturated part of the table) and the table's last index."""
    calls = np.array([[1, -1, 0]] + [[0, 2, 1], [-1, -1, -1], [1, 0, -1], [0, 1, 0], [1, 2, 1]], dtype=np.int8)
    quals = np.array([[0, 99, 157]] + [[30, 40, 0], [5, 6, 7], [157, 30, 200], [40, 40, 40], [40, 0, 30]], dtype=np.int16)
    counts = np.array([7, 1, 2, 3, 4, 5])
    nal = np.tile(np.array([2, 3, 2], dtype=np.int8), (3, 1))
    table = blockpath.qual_prob_table(0.01, 158)
    assert quals[calls >= 0].max() == len(table) - 1
    reads, rc = blockpath.expand_call_units(calls.reshape(-1), counts, [0, 1, 5], [0, 0, 3], [0, 0, 1], nal, 5, 3, error_rate=0.01,
                                            quals=quals.reshape(-1), quality_table=table)
    also, _ = blockpath.expand_call_units(calls.reshape(-1), counts, [0, 1, 5], [0, 0, 3], [0, 0, 1], nal, 5, 3, error_rate=0.01, quals=quals.reshape(-1))
    assert _same_bytes(reads, also)   # (the default table is the error rate's)
    t = lambda q: (table[q], (1.0 - table[q]) / 3.0)   # noqa: E731
    assert np.isnan(reads[0]).all() and rc[0].tolist() == [0] * 5
    (p0, o0), (p157, o157) = t(0), t(157)
    assert p0 == 0.0 and o0 == 1.0 / 3.0
    assert np.array_equal(reads[1, 0], [[o0, p0, 0.0], [np.nan, np.nan, np.nan], [p157, o157, 0.0]], equal_nan=True)
    assert np.isnan(reads[1, 1:]).all() and rc[1].tolist() == [7, 0, 0, 0, 0]
    assert np.array_equal(reads[2, 1], [[np.nan, np.nan, 0.0], [np.nan] * 3, [np.nan, np.nan, 0.0]], equal_nan=True)
    (p40, o40), (p30, o30) = t(40), t(30)
    assert np.array_equal(reads[2, 4], [[o40, p40, 0.0], [o0, o0, p0], [o30, p30, 0.0]]) and rc[2].tolist() == [1, 2, 3, 4, 5]
    for u, (a, b) in enumerate([(0, 0), (0, 1), (1, 6)]):
        want = encoding.encode_read_distributions([2, 3, 2], calls[a:b], quals[a:b], error_rate=0.01)
        assert _same_bytes(reads[u, : b - a], want.reshape(b - a, 3, 3))
    with pytest.raises(ValueError):   # (a called cell beyond the table)
        blockpath.expand_call_units(calls.reshape(-1), counts, [0, 1, 5], [0, 0, 3], [0, 0, 1], nal, 5, 3, quals=quals.reshape(-1), quality_table=table[:100])


def test_call_unit_inputs_carry_the_qualities():
    source = application.ReadSource(_pools(reference_bams(REFERENCE_JOBS[3][1]), "two"), use_phred=True)
    _, fast = _units_both_ways(os.path.join(HERE, REFERENCE_JOBS[3][0]), source)
    blk = fast[0]["block"]
    li = np.array([u["li"] for u in fast if len(u["locus"].positions) == len(fast[0]["locus"].positions)][::-1])
    for si in (np.zeros(len(li), dtype=np.int64), np.arange(len(li)) % 2):
        calls, counts, rows, c_off, n_off, nal, quals = blockpath.call_unit_inputs(blk["encs"], li, si, blk["nal"])
        assert quals.dtype == np.int16 and quals.shape == calls.shape and nal.shape == (len(li), len(fast[0]["locus"].positions))
        R, A = int(rows.max()), int(nal.max())
        reads, rc = blockpath.expand_call_units(calls, counts, rows, c_off, n_off, nal, R, A, error_rate=ERR, quals=quals, quality_table=blk["qtable"])
        for i, (l, s) in enumerate(zip(li, si)):
            sr = fast[int(l)]["reads"][source.samples[int(s)]]
            n = len(sr["counts"])
            assert n == rows[i] and _same_bytes(reads[i, :n, :, : sr["dists"].shape[2]], sr["dists"]) and rc[i, :n].tolist() == list(sr["counts"])
        compact = application._group_compact_reads(fast, [(int(l), source.samples[int(s)]) for l, s in zip(li, si)], R, A)
        assert compact.quals is not None and _same_bytes(np.asarray(compact), reads)


# ---- the gate, the keyword, the command line ----
@pytest.fixture(scope="module")
def synth_job(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wide_block"))
    job = synth.synth_assembly_inputs(d, n_loci=12, n_samples=3, reads_per_locus=14, n_snvs=5, gap=30)
    job["haps"] = haplotype_vcf(job, os.path.join(d, "haps.vcf"), specials=True)
    job["samples"] = ["S000", "S001", "S002"]
    a, b, c = zip(job["samples"], job["bams"])
    job["pools"] = {"P1": [a, b], "P2": [c, a]}
    return job


def test_which_sources_the_wide_gate_takes(synth_job):
    vcf = os.path.join(HERE, "simple.output.mixed_depth.assemble.vcf")
    paths = reference_bams(REFERENCE_JOBS[2][1])
    plain = application.ReadSource(paths)
    phred = application.ReadSource(paths, use_phred=True)
    pooled = application.ReadSource({"POOL": list(paths.items())})
    matrix = application.MatrixSource(SAMPLES, {}, use_phred=True)
    for source in (phred, pooled, matrix):
        assert not application._block_path_takes(source) and not sources._block_path_takes(source, wide=False)
        assert sources._block_path_takes(source, wide=True)
    assert sources._block_path_takes(plain) and sources._block_path_takes(plain, wide=True)
    # a pool without files, a file fetched region by region, a SAM text file: not even the wide gate
    empty = application.ReadSource({"POOL": list(paths.items())})
    empty.pools["NOBODY"] = []
    assert not sources._block_path_takes(empty, wide=True)
    fetched = application.ReadSource(synth_job["pools"], use_phred=True)
    assert sources._block_path_takes(fetched, wide=True)
    assert all(b.index is not None for b in fetched.bams.values())
    fetched.WHOLE_FILE_BYTES = 0
    assert not sources._block_path_takes(fetched, wide=True)
    for program in (application.call_exact, application.call):
        with pytest.raises(ValueError, match="block_path='wide'"):
            list(program(synth_job["haps"], fetched, block_path="wide"))
        with pytest.raises(ValueError, match="block_path"):
            list(program(vcf, phred, block_path="wider"))
    kw = dict(targets=io.read_bed4(synth_job["bed"]), ploidy=4, steps=60, burn=20, chains=2)
    with pytest.raises(ValueError, match="block_path='wide'"):
        list(application.assemble(None, synth_job["vcf"], io.Reference(synth_job["fasta"]), fetched, block_path="wide", **kw))
    with pytest.raises(ValueError, match="block_path='wide'"):   # (a custom sampler is evaluated locus by locus)
        list(application.assemble(None, synth_job["vcf"], io.Reference(synth_job["fasta"]), application.ReadSource(synth_job["pools"]),
                                  block_path="wide", sampler=_fake_sampler, **kw))
    # the keyword's other values mean what they meant
    for source in (phred, pooled):
        with pytest.raises(ValueError, match="block_path=True"):
            list(application.call_exact(vcf, source, block_path=True))


@pytest.mark.parametrize("kind", ["phred", "pooled", "pooled_phred"])
def test_call_exact_wide_reads_no_record_and_writes_the_same_lines(kind, synth_job):
    jobs = [(os.path.join(HERE, REFERENCE_JOBS[3][0]), reference_bams(REFERENCE_JOBS[3][1]), SAMPLES),
            (synth_job["haps"], dict(zip(synth_job["samples"], synth_job["bams"])), synth_job["samples"])]
    for vcf, paths, names in jobs:
        a, b, c = [(s, paths[s]) for s in names]
        source = application.ReadSource(paths if kind == "phred" else {"P1": [a, b], "P2": [c, a]}, use_phred=kind != "pooled")
        spy = _Spy(source)
        fast = list(application.call_exact(vcf, source, calling=_Replay, block_path="wide", report=("AFP",)))
        assert spy.n == 0 and len(fast) > 0
        assert list(application.call_exact(vcf, source, calling=_Replay, block_path="wide", records_per_block=3)) == \
            list(application.call_exact(vcf, source, calling=_Replay, block_path="wide")) and spy.n == 0
        slow = list(application.call_exact(vcf, source, calling=_Replay, block_path=False, report=("AFP",)))
        assert spy.n == len(fast) * len(source.samples) and slow == fast
        # None and False are what they were: record by record
        spy.n = 0
        assert list(application.call_exact(vcf, source, calling=_Replay, report=("AFP",))) == slow and spy.n == len(fast) * len(source.samples)


def test_a_negative_quality_sends_its_block_record_by_record(synth_job):
    bams = application.ReadSource(dict(zip(synth_job["samples"], synth_job["bams"])), use_phred=True)
    _, records = io.read_vcf(synth_job["haps"])
    units = application._exact_units(records, bams, bams.samples, None, None, False)
    matrices = {}
    for u in units:
        for s in bams.samples:
            chars, quals = io.extract_read_variants_columns(u["locus"], bams.bams[bams.pools[s][0][1]].columns(), s, as_codes=True, **bams.filter)
            matrices[(u["locus"].name, s)] = (chars, quals.copy())
    source = application.MatrixSource(bams.samples, matrices, use_phred=True)
    want = list(application.call_exact(synth_job["haps"], bams, calling=_Replay, block_path=False))
    spy = _Spy(source)
    assert list(application.call_exact(synth_job["haps"], source, calling=_Replay, block_path="wide", records_per_block=5)) == want and spy.n == 0
    # a negative quality in a called cell of the seventh record: the second block of five goes record by record
    u = units[6]
    calls, (chars, quals) = u["reads"]["S001"]["calls"], matrices[(u["locus"].name, "S001")]
    r, j = np.argwhere(calls >= 0)[0]
    quals[r, j] = -3
    source = application.MatrixSource(bams.samples, matrices, use_phred=True)
    spy = _Spy(source)
    slow = list(application.call_exact(synth_job["haps"], source, calling=_Replay, block_path=False))
    assert spy.n == len(want) * 3
    spy.n = 0
    assert list(application.call_exact(synth_job["haps"], source, calling=_Replay, block_path="wide", records_per_block=5)) == slow
    assert spy.n == 5 * 3


def _surrogate(dists, n_alleles):
    """int8 [*, M] rows that stand for a unit's float tensor in tests.test_blockpath._fake_summary (which keys its stand-in summary
    on the bytes of the rows it is given): gaps as -1, alleles a position does not have as 0 -- the all-gap row of a unit without
    reads is NaN throughout on the per-locus path and NaN, then 0, on the block path."""
    d = np.where(np.isnan(dists), -1.0, np.asarray(dists, dtype=np.float64))
    d = np.where(np.arange(d.shape[2])[None, None, :] >= np.asarray(n_alleles)[None, :, None], 0.0, d)
    M = d.shape[1]
    return np.frombuffer(np.ascontiguousarray(d.transpose(0, 2, 1)).tobytes(), dtype=np.int8).reshape(-1, M)


def _fake_sampler(units, settings):
    total = settings["chains"] * (settings["steps"] - settings["burn"])
    return [_as_dict(*_fake_summary(_surrogate(u["reads"], u["n_alleles"]), u["ploidy"], list(u["n_alleles"]), total), int(np.asarray(u["reads"]).shape[2]),
                     total=total) for u in units]


class _FakeQualBatch:
    """tests.test_blockpath._FakeBatch for from_calls with qualities: the stand-in summary of a unit is a function of the float
    tensor its calls and qualities expand to."""

    wph, MS, seen_quals = 1, 8, 0

    def __init__(self, model, calls, reads_off, n_reads, n_pos, max_allele, ploidy, counts, counts_off, n_alleles, nalleles_off,
                 inbreeding=None, error_rate=0.0024, quals=None):
        type(self).seen_quals += quals is not None
        self.model, self.K = model, int(ploidy.max())
        self.units_host = dict(fixed_off=np.cumsum(n_pos) - n_pos)
        self.res = []
        for u in range(len(n_reads)):
            R, M, A = int(n_reads[u]), int(n_pos[u]), int(max_allele[u])
            nal = np.asarray(n_alleles[nalleles_off[u]: nalleles_off[u] + M], dtype=np.int8)
            c = calls[reads_off[u]: reads_off[u] + R * M]
            q = None if quals is None else quals[reads_off[u]: reads_off[u] + R * M]
            d, _ = blockpath.expand_call_units(c, np.ones(R, dtype=np.int64), [R], [0], [0], nal[None, :], R, A, error_rate=error_rate, quals=q)
            self.res.append((_surrogate(d[0], nal), nal.tolist(), A))

    def run(self, burn, incongruence_threshold=0.6):
        self.total = self.model.chains * (self.model.steps - burn)

    def _all(self):
        return [_fake_summary(s, self.K, nal, self.total) + (A,) for s, nal, A in self.res]

    def summary_arrays(self):
        res = self._all()
        U, K = len(res), self.K
        a = dict(n=np.zeros(U, dtype=np.int32), stats=np.zeros((U, 2)), mode_words=np.zeros((U, K), dtype=np.uint64), mci=np.zeros(U, dtype=np.int32),
                 status=np.zeros(U, dtype=np.int32), total=self.total)
        for u, (w, c, fx, spm, gpm, mw, mci, plain, A) in enumerate(res):
            a["n"][u] = len(w) if plain else -1
            a["stats"][u], a["mode_words"][u], a["mci"][u] = (spm, gpm), mw, mci
        a["fixed"] = np.concatenate([r[2] for r in res])
        a["plain"] = a["n"] >= 0
        a["words"] = np.concatenate([r[0] for r in res if r[7]] + [np.zeros((0, K), dtype=np.uint64)])
        a["counts"] = np.concatenate([r[1] for r in res if r[7]] + [np.zeros(0, dtype=np.int32)])
        return a

    def results(self, raise_on_limit=True, only=None):
        res = self._all()
        return [_as_dict(*res[u], total=self.total) for u in (range(len(res)) if only is None else only)]


@pytest.mark.parametrize("kind", ["phred", "pooled", "pooled_phred"])
@pytest.mark.parametrize("report", [(), ("AFP", "GP", "SNVDP")])
def test_assemble_wide_reads_no_locus_and_writes_the_same_lines(kind, report, synth_job, monkeypatch):
    paths = dict(zip(synth_job["samples"], synth_job["bams"]))
    use_phred = kind != "pooled"
    make = lambda: application.ReadSource(paths if kind == "phred" else synth_job["pools"], use_phred=use_phred)   # noqa: E731
    samples = make().samples
    targets = io.read_bed4(synth_job["bed"])
    targets.append(("chrS", 3, 9, "no_snvs"))
    _, variants = io.read_vcf(synth_job["vcf"])
    variants.append(dict(chrom="chrS", pos=20, id=".", ref="A", alts=("C",), info={}))   # an SNV nobody covers (no reads: one gap row)
    targets.append(("chrS", 15, 25, "snv_without_reads"))
    ref = io.Reference(synth_job["fasta"])
    kw = dict(ploidy={s: (2 if i else 4) for i, s in enumerate(samples)}, inbreeding=0.1, steps=60, burn=20, chains=2, report=report, targets=targets)
    slow = list(application.assemble(None, variants, ref, make(), sampler=_fake_sampler, block_path=False, **kw))
    source = make()
    spy = _Spy(source)
    monkeypatch.setattr(_FakeQualBatch, "seen_quals", 0)
    fast = list(application.assemble(None, variants, ref, source, block_path="wide", _batch_factory=_FakeQualBatch, **kw))
    assert spy.n == 0 and (_FakeQualBatch.seen_quals > 0) == use_phred
    assert len(fast) == len(targets) and fast == slow
    again = list(application.assemble(None, variants, ref, source, block_path="wide", _batch_factory=_FakeQualBatch, units_per_block=len(samples) * 5, **kw))
    assert again == fast and spy.n == 0


def test_command_line_flag_and_the_new_symbol():
    for program in ("assemble", "call", "call-exact"):
        parser = cli.build_parser(program)
        assert parser.parse_args([]).block_path == "auto"
        for text, value in (("auto", None), ("off", False), ("on", True), ("wide", "wide")):
            assert cli.BLOCK_PATHS[parser.parse_args(["--block-path", text]).block_path] is value or value == "wide"
        assert cli.BLOCK_PATHS[parser.parse_args(["--block-path", "wide"]).block_path] == "wide"
        with pytest.raises(SystemExit):
            parser.parse_args(["--block-path", "fast"])
    with pytest.raises(SystemExit):
        cli.build_parser("find-snvs").parse_args(["--block-path", "wide"])
    from mchap_amd import _lib

    name = "mchap_call_reads_from_calls_quals_device"
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mchap_hip.h")).read()
    assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header)
