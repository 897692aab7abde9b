"""Where the programs' reads come from: alignment files (ReadSource) or pileup matrices the caller has already (MatrixSource),
the per-locus read encoding (application/baseclass.py:140-210) and the encoding of a whole block of loci at once
(mchap_amd/blockpath.py) that `assemble`, `call` and `call-exact` share."""
import numpy as np

from . import encoding
from .io import extract_read_variants, read_alignments


READ_FILTER = dict(min_quality=20, skip_duplicates=True, skip_qcfail=True, skip_supplementary=True)


class ReadSource:
    """The alignment files of a run, each read once, and the read encoding settings (application/baseclass.py:48-57).
    sample_bams: ordered {sample: path}, or {pool: [(sample, path), ...]} when samples are pooled (--sample-pool: a pool's
    reads are those of its samples, concatenated: baseclass.py:153-187)."""

    def __init__(self, sample_bams, error_rate=0.0024, use_phred=False, read_group_field="SM", mapping_quality=20,
                 skip_duplicates=True, skip_qcfail=True, skip_supplementary=True, workers=1):
        self.pools = {k: ([(k, v)] if isinstance(v, str) else list(v)) for k, v in sample_bams.items()}
        self.samples = list(self.pools)
        self.error_rate, self.use_phred = error_rate, use_phred
        self.filter = dict(min_quality=mapping_quality, skip_duplicates=skip_duplicates, skip_qcfail=skip_qcfail,
                           skip_supplementary=skip_supplementary)
        paths = list(dict.fromkeys(p for pairs in self.pools.values() for _, p in pairs))
        self.workers = int(workers)
        self.id_field = read_group_field

        def load(q):
            # BAM: block-wise reader with columnar records (and region fetches through the .bai index for big files);
            # SAM text: the record reader
            with open(q, "rb") as f:
                magic = f.read(2)
            if magic == b"\x1f\x8b":
                from .io import BamFile

                return BamFile(q, read_group_field, workers=self.workers)
            return read_alignments(q, read_group_field)

        if workers > 1 and len(paths) > 1:
            # --cores: the files are read by a pool of threads (zlib releases the interpreter lock)
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max_workers=int(workers)) as ex:
                loaded = list(ex.map(load, paths))
        else:
            loaded = [load(q) for q in paths]
        self.bams = dict(zip(paths, loaded))

    WHOLE_FILE_BYTES = 256 << 20  # smaller files are inflated once; bigger ones are fetched region by region (needs the .bai)

    def reads(self, locus, sample):
        from .io import BamFile, extract_read_variants_columns

        M = len(locus.positions)
        parts = []
        for name, path in self.pools[sample]:
            bam = self.bams[path]
            if isinstance(bam, BamFile):
                region = bam.index is not None and len(bam.data) > self.WHOLE_FILE_BYTES
                cols = bam.columns(locus.contig, locus.start, locus.stop) if region else bam.columns()
                parts.append(extract_read_variants_columns(locus, cols, name, as_codes=True, **self.filter))
            else:
                c, q = extract_read_variants(locus, bam, name, **self.filter)
                parts.append((_codes(c), q))
        if parts:
            chars, quals = np.concatenate([c for c, _ in parts]), np.concatenate([q for _, q in parts])
        else:
            chars, quals = np.empty((0, M), dtype=np.uint8), np.empty((0, M), dtype=np.int16)
        return encode_reads(locus, chars, quals, self.error_rate, self.use_phred)


class MatrixSource:
    """Reads given as what extract_read_variants yields -- {(target name, sample): (chars [n_reads, n_snv] as str or uint8
    ASCII codes, summed base qualities [n_reads, n_snv])} -- instead of alignment files: a caller that has its pileups
    already (and the docs/example fixture of the tests and of bench.py's extra.config1)."""

    def __init__(self, samples, matrices, error_rate=0.0024, use_phred=False):
        self.samples = list(samples)
        self.matrices = matrices
        self.error_rate, self.use_phred = error_rate, use_phred
        self.bams = {}
        self._codes = {}

    def codes(self, name, sample):
        """(characters as uint8 ASCII codes, qualities as int16) of a (target, sample): converted once."""
        key = (name, sample)
        got = self._codes.get(key)
        if got is None:
            chars, quals = self.matrices[key]
            got = self._codes[key] = (_codes(chars), np.asarray(quals, dtype=np.int16))
        return got

    def reads(self, locus, sample):
        chars, quals = self.matrices[(locus.name, sample)]
        return encode_reads(locus, np.asarray(chars), np.asarray(quals, dtype=np.int16), self.error_rate, self.use_phred)


def load_matrices(path):
    """A pileup file written as numpy .npz (tests/golden/make_example_fixture.py documents the layout: samples, contigs,
    targets, per target its SNV positions and alleles, per (target, sample) the character matrix and the qualities) ->
    (samples, targets [(contig, start, stop, name)], variant records, {(target name, sample): (chars, quals)},
    contigs [(name, length)])."""
    z = np.load(path)
    samples = [str(x) for x in z["samples"]]
    targets = [(str(c), int(a), int(b), str(n)) for c, a, b, n in zip(z["target_contig"], z["target_start"], z["target_stop"], z["target_name"])]
    variants, matrices = [], {}
    for li, (contig, start, stop, name) in enumerate(targets):
        for p, al in zip(z["pos_%d" % li], z["alleles_%d" % li]):
            al = str(al)
            variants.append(dict(chrom=contig, pos=int(p) + 1, id=".", ref=al[0], alts=tuple(al[1:]), info={}))
        for si, s_ in enumerate(samples):
            matrices[(name, s_)] = (z["chars_%d_%d" % (li, si)], z["quals_%d_%d" % (li, si)])
    contigs = [(str(c), int(n)) for c, n in zip(z["contigs"], z["contig_lengths"])]
    return samples, targets, variants, matrices, contigs


def sample_reads(locus, pairs, error_rate=0.0024, use_phred=False, read_filter=None):
    """encode_sample_reads (application/baseclass.py:140-210) for one sample (or pool): pairs = [(read-group sample name,
    alignment as read_alignments returns it), ...] -> dict(chars, calls, depth, dists (distinct rows), counts)."""
    M = len(locus.positions)
    parts = [extract_read_variants(locus, bam, name, **(read_filter or READ_FILTER)) for name, bam in pairs]
    if parts:
        chars, quals = np.concatenate([c for c, _ in parts]), np.concatenate([q for _, q in parts])
    else:
        chars, quals = np.empty((0, M), dtype=np.uint8), np.empty((0, M), dtype=np.int16)
    return encode_reads(locus, chars, quals, error_rate, use_phred)


def _codes(chars):
    """A character matrix ('U1' strings, or uint8 ASCII codes already) as uint8 ASCII codes."""
    chars = np.asarray(chars)
    if chars.dtype == np.uint8:
        return chars
    return chars.astype("S1").view(np.uint8).reshape(chars.shape) if chars.size else np.empty(chars.shape, dtype=np.uint8)


def encode_reads(locus, chars, quals, error_rate=0.0024, use_phred=False):
    """Character matrix (strings or ASCII codes) + qualities -> allele calls, probabilistic rows, de-duplicated rows with
    counts, depth (application/baseclass.py:189-207)."""
    M = len(locus.positions)
    chars = _codes(chars)
    calls = np.full(chars.shape, -1, dtype=np.int8)
    if M and chars.shape[0]:
        # allele index of every character: one table look-up per SNV column
        lut = np.full((M, 256), -1, dtype=np.int8)
        for j in range(M):
            for a, c in enumerate(locus.alleles[j]):
                if lut[j, ord(c)] < 0:
                    lut[j, ord(c)] = a
        calls = lut[np.arange(M)[None, :], chars]
    if use_phred or M == 0 or calls.shape[0] == 0:
        dists = encoding.encode_read_distributions(locus.n_alleles, calls, quals if use_phred else None, error_rate=error_rate)
        uniq, counts = encoding.unique_counts(dists)
    else:
        # qualities ignored: a row of distributions is a function of its row of calls, so the distinct rows (in order of first
        # appearance, with their counts: mset.unique_counts at application/baseclass.py:207) are found on the int8 calls and
        # only those are turned into distributions
        ucalls, counts = encoding.unique_counts(np.ascontiguousarray(calls))
        uniq = encoding.encode_read_distributions(locus.n_alleles, ucalls, None, error_rate=error_rate)
    depth = (chars != ord("-")).sum(axis=0) if M else np.array([])
    return dict(chars=chars, calls=calls, depth=depth, dists=uniq, counts=counts)


def _block_path_takes(source, wide=False):
    """The array path of a block reads every sample from one alignment file held whole in memory (or from pileup matrices the
    caller has already), base qualities ignored.  wide (block_path="wide"): base qualities in use and pooled samples -- every
    pool one or more (read group, file) pairs -- are taken too; the files still have to be BAM files held whole."""
    from .io import BamFile

    if wide:
        if isinstance(source, MatrixSource):
            return True
        if not isinstance(source, ReadSource):
            return False
        for pairs in source.pools.values():
            if len(pairs) < 1:
                return False
            for _, path in pairs:
                bam = source.bams[path]
                if not isinstance(bam, BamFile) or (bam.index is not None and len(bam.data) > source.WHOLE_FILE_BYTES):
                    return False
        return True
    if isinstance(source, MatrixSource):
        return not source.use_phred
    if not isinstance(source, ReadSource) or source.use_phred:
        return False
    for pairs in source.pools.values():
        if len(pairs) != 1:
            return False
        bam = source.bams[pairs[0][1]]
        if not isinstance(bam, BamFile) or (bam.index is not None and len(bam.data) > source.WHOLE_FILE_BYTES):
            return False
    return True


def _block_encodings(loci, source, samples, timings=None, inflate_together=False):
    """blockpath.extract_block / encode_block over the loci of a block (records of call / call-exact, targets of assemble), once per
    sample (tables and look-up table shared): dict(encs [per sample], si {sample: index}, nal int8 alleles of every SNV, tables,
    error_rate, qtable).  A pooled sample's pile is its pairs' piles concatenated (blockpath.concat_piles; a (read group, file) pair
    shared by several pools is extracted once); qtable: blockpath.qual_prob_table over the block's qualities when the source uses
    them (the rows are then de-duplicated as their float rows are), else None.  timings: a dict whose "bam_parse_s" receives the seconds spent inflating and parsing files on their first use;
    inflate_together: files not parsed yet are inflated and walked side by side when the source has workers for it."""
    import time as _time

    from . import blockpath as bp

    tables = bp.locus_tables(loci)
    n_snv = int(tables[1][-1])
    lut = bp.allele_lut(loci, n_snv)

    def parsed(since):
        if timings is not None:
            timings["bam_parse_s"] = timings.get("bam_parse_s", 0.0) + _time.perf_counter() - since

    if inflate_together and isinstance(source, ReadSource) and source.workers > 1:
        # (zlib and the library's record walk release the interpreter lock)
        todo = [b for b in dict.fromkeys(source.bams[path] for s_ in samples for _, path in source.pools[s_]) if getattr(b, "_all", 0) is None]
        if len(todo) > 1:
            from concurrent.futures import ThreadPoolExecutor

            tp = _time.perf_counter()
            with ThreadPoolExecutor(max_workers=min(source.workers, len(todo))) as ex:
                list(ex.map(lambda b: b.columns(), todo))
            parsed(tp)
    extracted = {}

    def pair_pile(name, path):
        got = extracted.get((name, path))
        if got is None:
            tp = _time.perf_counter()
            cols = source.bams[path].columns()   # (the first use of a file inflates and parses it)
            parsed(tp)
            got = extracted[(name, path)] = bp.extract_block(loci, cols, name, tables=tables, **source.filter)
        return got

    piles = []
    for sample in samples:
        if isinstance(source, MatrixSource):
            piles.append(bp.pile_from_matrices(loci, [source.codes(l.name, sample) for l in loci], tables=tables))
        else:
            piles.append(bp.concat_piles([pair_pile(name, path) for name, path in source.pools[sample]]))
    qtable = None
    if source.use_phred:
        qtable = bp.qual_prob_table(source.error_rate, max((int(p.quals.max(initial=0)) for p in piles), default=0) + 1)
    encs = [bp.encode_block(loci, pile, lut, **({} if qtable is None else dict(quality_table=qtable))) for pile in piles]
    nal = np.fromiter((a for l in loci for a in l.n_alleles), dtype=np.int8, count=n_snv)
    return dict(encs=encs, si={s: i for i, s in enumerate(samples)}, nal=nal, tables=tables, error_rate=source.error_rate, qtable=qtable)
