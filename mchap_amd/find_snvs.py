"""`find-snvs`: candidate SNVs from read pileups (reference application/find_snvs.py: bam_region_depths, write_vcf_block).

The per-base histogram over (position x sample x 4 bases) and the allele filter over it run on the GPU
(csrc/pileup_kernel.hpp); the host builds the tables the kernels read, with array operations over AlignmentColumns:
  - per sample, the aligned (M/=/X) runs of the reads that pass the read filters, clipped to the block's target windows and
    to tiles of target rows, indexed CSR by (sample, tile);
  - the mate pairs of htslib's overlap rule and the reference positions both mates align a base to.
Only the rows the filter keeps come back to the host.  Counting rule, and where it departs from the reference: DESIGN.md
"find-snvs".  Optionally (`genotypes=`, not in the reference) a fourth launch calls every sample's genotype at every record from the
depth tensor (csrc/snv_genotype_kernel.hpp) and the records carry GT:GPM:AD.  There is no CPU path: a missing library or device is an error."""
import ctypes as C
import time

import numpy as np

from . import io

MIN_BASE_QUALITY = 13   # pysam's pileup default (min_base_quality)
TILE = 2048             # target rows per depth workgroup (its LDS histogram: TILE x 4 u32)
ACGT = np.array(list("ACGT"))
_REF_INDEX = np.full(256, -1, dtype=np.int8)
for _i, _c in enumerate("ACGT"):
    _REF_INDEX[ord(_c)] = _REF_INDEX[ord(_c.lower())] = _i


def bases_to_indices(seq):
    """A reference sequence (str) -> int8 allele indices, A C G T (either case) 0-3, anything else -1."""
    return _REF_INDEX[np.frombuffer(seq.encode(), dtype=np.uint8)] if seq else np.zeros(0, dtype=np.int8)


def read_targets(path):
    """The intervals of a BED file (3+ columns, 0-based half-open) in file order, repeats and overlaps kept."""
    out = []
    for line in io.open_text(path):
        f = line.split()
        if len(f) < 3 or f[0].startswith("#") or f[0] in ("track", "browser"):
            continue
        out.append((f[0], int(f[1]), int(f[2])))
    return out


def check_one_sample_per_file(sample_bams, id_field="SM"):
    """The reference's bam_samples: a file whose read groups name more than one sample is refused."""
    for path in dict.fromkeys(sample_bams.values()):
        rg = io.bam_header(path)[1]
        names = list(dict.fromkeys(rg if id_field == "ID" else rg.values()))
        if len(names) > 1:
            raise ValueError("Expected one sample per bam but found {} and {} in {}".format(names[0], names[1], path))


# ---- host tables ------------------------------------------------------------------------------------------------------
def _ramp(counts):
    """0..c-1 for each count c, concatenated."""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    return np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)


def _aligned(cols, recs):
    """The M/=/X operations of the given records: (owner index into recs, reference start, length, read start)."""
    recs = np.asarray(recs, dtype=np.int64)
    n_cig = cols.seg_first[recs + 1] - cols.seg_first[recs]
    idx = np.repeat(cols.seg_first[recs], n_cig) + _ramp(n_cig)
    owner = np.repeat(np.arange(len(recs), dtype=np.int64), n_cig)
    op = cols.c_op[idx]
    m = ((op == 0) | (op == 7) | (op == 8)) & (cols.c_len[idx] > 0)
    idx = idx[m]
    return owner[m], cols.c_ref0[idx], cols.c_len[idx], cols.c_read0[idx]


def passing_records(cols, tid, lo_pos, hi_pos, min_quality=20, skip_duplicates=True, skip_qcfail=True, skip_supplementary=True):
    """Indices (file order) of the records of reference `tid` overlapping [lo_pos, hi_pos) that the pileup counts: the read
    filters of application.ReadSource (its `filter` keywords: unmapped, secondary, MAPQ < min_quality, and duplicate / qcfail / supplementary unless kept) plus
    pysam's orphan rule (paired, not a proper pair)."""
    if cols.n == 0 or tid < 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = cols.window(tid, lo_pos, hi_pos)
    r = np.arange(lo, hi, dtype=np.int64)
    fl = cols.flag[r]
    skip = 0x4 | 0x100 | (0x400 if skip_duplicates else 0) | (0x200 if skip_qcfail else 0) | (0x800 if skip_supplementary else 0)
    orphan = ((fl & 0x1) != 0) & ((fl & 0x2) == 0)
    ok = (cols.ref_id[r] == tid) & ((fl & skip) == 0) & ~orphan & (cols.mapq[r] >= min_quality) & \
        (cols.pos[r] < hi_pos) & (cols.end[r] > lo_pos)
    return r[ok]


def mate_pairs(cols, recs):
    """htslib's overlap pairing (bam_plp overlap_push) over the records `recs` (file order): a record that is a proper pair with
    its mate mapped on the same reference waits for its mate when the mate lies at or after it; the next record of the same
    name met while the first is still under the pileup (it starts before the first one ends) forms the pair (first, second).
    -> (first, second) record index arrays; every record is in at most one pair."""
    recs = np.asarray(recs, dtype=np.int64)
    fl = cols.flag[recs]
    el = recs[((fl & 0x2) != 0) & ((fl & 0x8) == 0) & (cols.next_ref_id[recs] == cols.ref_id[recs])]
    if len(el) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    q = cols.qname[el]
    order = np.argsort(q, kind="stable")
    qs = q[order]
    starts = np.r_[True, qs[1:] != qs[:-1]]
    gid = np.cumsum(starts) - 1
    size = np.bincount(gid)
    waits = lambda r: (cols.next_pos[r] >= cols.pos[r]) | (((cols.flag[r] & 1) != 0) & (cols.next_pos[r] == -1))  # noqa: E731
    # names met exactly twice: one array step
    two = size[gid] == 2
    a = el[order[two & starts]]
    b = el[order[two & ~starts]]
    ok = waits(a) & (cols.pos[b] < cols.end[a])
    A, B = [a[ok]], [b[ok]]
    # names met three times or more (supplementary alignments kept): the hash walked record by record
    for g in np.flatnonzero(size > 2):
        members = el[order[gid == g]]
        held = -1
        for r in members:
            if held >= 0 and cols.pos[r] >= cols.end[held]:
                held = -1  # the held read left the pileup before this one arrived
            if held < 0:
                if waits(np.array([r]))[0]:
                    held = int(r)
            else:
                A.append(np.array([held]))
                B.append(np.array([r]))
                held = -1
    return np.concatenate(A).astype(np.int64), np.concatenate(B).astype(np.int64)


def overlap_segments(cols, first, second):
    """The runs of reference positions where both mates of a pair align a base (M/=/X), as int64 [n][5] = {first's sequence
    nibble, second's sequence nibble, first's quality byte, second's quality byte, length} in the coordinates of cols.buf."""
    K = len(first)
    if K == 0:
        return np.zeros((0, 5), dtype=np.int64)
    oa, ra, la, da = _aligned(cols, first)
    ob, rb, lb, db = _aligned(cols, second)
    nb = np.bincount(ob, minlength=K)
    fb = np.cumsum(nb) - nb
    rep = nb[oa]
    i = np.repeat(np.arange(len(oa)), rep)
    j = np.repeat(fb[oa], rep) + _ramp(rep)
    x0 = np.maximum(ra[i], rb[j])
    x1 = np.minimum(ra[i] + la[i], rb[j] + lb[j])
    m = x1 > x0
    i, j, x0, x1 = i[m], j[m], x0[m], x1[m]
    a_ro = da[i] + (x0 - ra[i])
    b_ro = db[j] + (x0 - rb[j])
    ra_, rb_ = first[oa[i]], second[ob[j]]
    return np.stack([2 * cols.seq_off[ra_] + a_ro, 2 * cols.seq_off[rb_] + b_ro, cols.qual_off[ra_] + a_ro,
                     cols.qual_off[rb_] + b_ro, x1 - x0], axis=1).astype(np.int64)


def segment_table(cols, tid, starts, stops, rows, read_filter=None):
    """The pileup tables of one sample for a block of target windows on reference `tid` (window k covers [starts[k], stops[k])
    and block rows rows[k] ..): -> dict(
        segments int64 [n][4] = {block row, length, sequence nibble, quality byte}: an aligned run of a counted read clipped to
                 one window (coordinates of cols.buf),
        overlaps int64 [m][5] (overlap_segments of the counted reads' mate pairs),
        run (lo, hi): the byte range of cols.buf holding every counted record)."""
    starts, stops, rows = (np.asarray(x, dtype=np.int64) for x in (starts, stops, rows))
    empty = dict(segments=np.zeros((0, 4), np.int64), overlaps=np.zeros((0, 5), np.int64), run=(0, 0))
    if len(starts) == 0:
        return empty
    recs = passing_records(cols, tid, int(starts.min()), int(stops.max()), **(read_filter or {}))
    if len(recs) == 0:
        return empty
    owner, g0, gl, gr = _aligned(cols, recs)
    o = np.argsort(g0, kind="stable")
    owner, g0, gl, gr = owner[o], g0[o], gl[o], gr[o]
    L = int(gl.max()) if len(gl) else 1
    lo_k = np.searchsorted(g0, starts - L + 1, side="left")
    hi_k = np.searchsorted(g0, stops, side="left")
    cnt = np.maximum(hi_k - lo_k, 0)
    tk = np.repeat(np.arange(len(starts)), cnt)
    gk = np.repeat(lo_k, cnt) + _ramp(cnt)
    x0 = np.maximum(g0[gk], starts[tk])
    x1 = np.minimum(g0[gk] + gl[gk], stops[tk])
    m = x1 > x0
    tk, gk, x0, x1 = tk[m], gk[m], x0[m], x1[m]
    rec = recs[owner[gk]]
    ro = gr[gk] + (x0 - g0[gk])
    seg = np.stack([rows[tk] + (x0 - starts[tk]), x1 - x0, 2 * cols.seq_off[rec] + ro, cols.qual_off[rec] + ro], axis=1)
    used = np.unique(rec)
    a, b = mate_pairs(cols, used)
    off = cols.offsets[used]
    size = np.ascontiguousarray(cols.buf[off[:, None] + np.arange(4)]).view("<i4").reshape(-1).astype(np.int64)
    return dict(segments=seg.astype(np.int64), overlaps=overlap_segments(cols, a, b), run=(int(off.min()), int((off + 4 + size).max())))


def tile_index(segments, sample, n_samples, n_rows, tile):
    """Segments split at tile boundaries and ordered CSR by (sample, tile): -> (segments [n][4], tile_first [S x n_tiles + 1])."""
    seg = np.asarray(segments, dtype=np.int64).reshape(-1, 4)
    smp = np.asarray(sample, dtype=np.int64)
    n_tiles = (n_rows + tile - 1) // tile
    t0 = seg[:, 0] // tile
    t1 = (seg[:, 0] + seg[:, 1] - 1) // tile
    k = t1 - t0 + 1
    i = np.repeat(np.arange(len(seg)), k)
    t = np.repeat(t0, k) + _ramp(k)
    a = np.maximum(seg[i, 0], t * tile)
    e = np.minimum(seg[i, 0] + seg[i, 1], (t + 1) * tile)
    d = a - seg[i, 0]
    out = np.stack([a, e - a, seg[i, 2] + d, seg[i, 3] + d], axis=1)
    key = smp[i] * n_tiles + t
    o = np.argsort(key, kind="stable")
    first = np.zeros(n_samples * n_tiles + 1, dtype=np.int64)
    first[1:] = np.cumsum(np.bincount(key, minlength=n_samples * n_tiles))
    return np.ascontiguousarray(out[o]), first


# ---- device ----------------------------------------------------------------------------------------------------------
def _lib():
    from . import _lib as L

    return L, L.lib()


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class _Files:
    """The alignment file of every sample of a ReadSource (one file per sample), read as AlignmentColumns."""

    def __init__(self, source):
        self.source = source
        self.samples = list(source.samples)
        self.paths = []
        for s in self.samples:
            pairs = source.pools[s]
            if len(pairs) != 1:
                raise ValueError("find-snvs takes one alignment file per sample (no pools): %s" % s)
            self.paths.append(pairs[0][1])
        self._sam = {}

    def columns(self, i, contig, lo, hi):
        bam = self.source.bams[self.paths[i]]
        if isinstance(bam, io.BamFile):
            region = bam.index is not None and len(bam.data) > self.source.WHOLE_FILE_BYTES
            return bam.columns(contig, lo, hi) if region else bam.columns()
        path = self.paths[i]
        if path not in self._sam:
            self._sam[path] = io.sam_columns(path, self.source.id_field)
        return self._sam[path]


def _block_depths(files, windows, tile=TILE, variant=0, timings=None):
    """One block: windows [(contig, start, stop)] on ONE contig -> depth int32 [rows, S, 4] on the device (overlap tweak and
    histogram launches enqueued on the current stream)."""
    import torch

    _, L = _lib()
    S = len(files.samples)
    contig = windows[0][0]
    starts = np.array([w[1] for w in windows], dtype=np.int64)
    stops = np.array([w[2] for w in windows], dtype=np.int64)
    rows0 = np.r_[0, np.cumsum(stops - starts)[:-1]].astype(np.int64)
    n_rows = int((stops - starts).sum())
    t0 = time.perf_counter()
    segs, ovs, smp, chunks, base = [], [], [], [], 0
    t_inflate = 0.0
    for i in range(S):
        ti = time.perf_counter()
        cols = files.columns(i, contig, int(starts.min()), int(stops.max()))
        t_inflate += time.perf_counter() - ti
        names = [n for n, _ in cols.refs]
        tid = names.index(contig) if contig in names else -1
        tab = segment_table(cols, tid, starts, stops, rows0, files.source.filter)
        lo, hi = tab["run"]
        if hi > lo:
            chunks.append(np.asarray(cols.buf[lo:hi]))
            d = base - lo  # rebase onto the block's byte buffer
            sg, ov = tab["segments"].copy(), tab["overlaps"].copy()
            sg[:, 2] += 2 * d
            sg[:, 3] += d
            ov[:, 0:2] += 2 * d
            ov[:, 2:4] += d
            segs.append(sg)
            ovs.append(ov)
            smp.append(np.full(len(sg), i, dtype=np.int64))
            base += hi - lo
    seg = np.concatenate(segs) if segs else np.zeros((0, 4), np.int64)
    ov = np.concatenate(ovs) if ovs else np.zeros((0, 5), np.int64)
    seg_t, tile_first = tile_index(seg, np.concatenate(smp) if smp else np.zeros(0, np.int64), S, n_rows, tile)
    ov_first = np.r_[0, np.cumsum(ov[:, 4])].astype(np.int64)
    buf = np.concatenate(chunks) if chunks else np.zeros(16, np.uint8)
    if timings is not None:
        timings["inflate"] = timings.get("inflate", 0.0) + t_inflate
        timings["tables"] = timings.get("tables", 0.0) + (time.perf_counter() - t0 - t_inflate)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_buf = torch.from_numpy(buf).to(dev)
    d_seg = torch.from_numpy(seg_t).to(dev)
    d_first = torch.from_numpy(tile_first).to(dev)
    d_ov = torch.from_numpy(np.ascontiguousarray(ov[:, :4])).to(dev)
    d_ovf = torch.from_numpy(ov_first).to(dev)
    depth = (torch.zeros if variant == 1 else torch.empty)((n_rows, S, 4), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = _events(timings)
    from ._lib import check

    check(L.mchap_pileup_overlap_device(_vp(d_buf), d_buf.numel(), _vp(d_ov), _vp(d_ovf), len(ov), int(ov_first[-1]), stream))
    check(L.mchap_pileup_depth_device(_vp(d_buf), d_buf.numel(), _vp(d_seg), _vp(d_first), S, n_rows, int(tile), MIN_BASE_QUALITY,
                                      int(variant), _vp(depth), stream))
    if ev is not None:
        ev[1].record()
        timings.setdefault("_events", []).append(("depth", ev[0], ev[1]))
    return depth, rows0


def _events(timings):
    if timings is None:
        return None
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0, e1


def allele_depths(source, contig, start, stop, tile=TILE, variant=0):
    """Per-base allele depths of [start, stop) of `contig`: int64 [stop - start, n_samples, 4] (A C G T), counted on the device
    by the pileup kernels -- the analogue of the reference's bam_region_depths."""
    import torch

    files = _Files(source)
    depth, _ = _block_depths(files, [(contig, int(start), int(stop))], tile=tile, variant=variant)
    torch.cuda.current_stream().synchronize()
    return depth.cpu().numpy().astype(np.int64)


def filter_device(depth, ref_index, maf=0.0, mad=0, ind_maf=0.1, ind_mad=3, min_ind=1):
    """The filter launch over a device depth tensor int32 [P, S, 4] and int8 reference indices [P]: -> (flags int32 [P],
    admf float64 [P, 4]) on the device (layout: include/mchap_hip.h mchap_pileup_filter_device)."""
    import torch

    from ._lib import check

    _, L = _lib()
    P, S = int(depth.shape[0]), int(depth.shape[1])
    depth = depth.contiguous()
    ref_index = ref_index.to(device=depth.device, dtype=torch.int8).contiguous()
    flags = torch.empty(P, dtype=torch.int32, device=depth.device)
    admf = torch.empty((P, 4), dtype=torch.float64, device=depth.device)
    check(L.mchap_pileup_filter_device(_vp(depth), _vp(ref_index), P, S, float(maf), int(mad), float(ind_maf), int(ind_mad), int(min_ind),
                                       _vp(flags), _vp(admf), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return flags, admf


def decode_flags(flags):
    """flags of the filter launch -> (record bool [n], keep bool [n, 4] by allele index, order int [n, 4], refmasked bool [n])."""
    flags = np.asarray(flags, dtype=np.int64)
    keep = ((flags[:, None] >> (1 + np.arange(4))) & 1).astype(bool)
    order = (flags[:, None] >> (8 + 2 * np.arange(4))) & 3
    return (flags & 1).astype(bool), keep, order, ((flags >> 16) & 1).astype(bool)


def genotypes_device(depth, flags, admf, ploidy, inbreeding=None, frequencies=None, error_rate=0.0024):
    """Genotype calls over the tensors the depth and filter launches leave on the device (the rule: include/mchap_hip.h
    mchap_snv_genotypes_device): depth int32 [P, S, 4], flags int32 [P], admf float64 [P, 4].  ploidy: one value or one
    per sample; inbreeding: None (no prior unless frequencies are asked for, which then means 0), one value or one per sample
    (NaN: no prior for that sample); frequencies: None or "ADMF".  -> (gt_index int32 [P, S], gpm float64 [P, S]) on the device:
    the mode's index among the genotypes over the row's enumerated alleles and its posterior probability, -1 / NaN for a row that
    is no record and for a no-call."""
    import torch

    from ._lib import check

    _, L = _lib()
    if frequencies not in (None, "ADMF"):
        raise ValueError('frequencies must be None or "ADMF"')
    if not 0.0 <= float(error_rate) < 1.0:
        raise ValueError("error_rate must be in [0, 1)")
    P, S = int(depth.shape[0]), int(depth.shape[1])
    k = np.broadcast_to(np.asarray(ploidy, dtype=np.int64), (S,))
    if inbreeding is None:
        inbreeding = 0.0 if frequencies == "ADMF" else np.nan
    F = np.broadcast_to(np.asarray(inbreeding, dtype=np.float64), (S,))
    if ((F < 0) | (F >= 1)).any():
        raise ValueError("inbreeding must be in [0, 1)")
    depth, flags, admf = depth.contiguous(), flags.contiguous(), admf.contiguous()
    d_k = torch.from_numpy(k.astype(np.int32)).to(depth.device)
    d_F = torch.from_numpy(np.array(F, dtype=np.float64)).to(depth.device)
    gt = torch.empty((P, S), dtype=torch.int32, device=depth.device)
    gpm = torch.empty((P, S), dtype=torch.float64, device=depth.device)
    p_call = 1.0 - float(error_rate)      # (as encoding.encode_read_distributions forms them)
    p_other = (1.0 - p_call) / 3.0
    check(L.mchap_snv_genotypes_device(_vp(depth), _vp(flags), _vp(admf), P, S, _vp(d_k), _vp(d_F), int(frequencies == "ADMF"),
                                       C.c_double(p_call), C.c_double(p_other), _vp(gt), _vp(gpm),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return gt, gpm


def genotype_alleles(index, ploidy, refmasked=False):
    """A genotype index over a record's enumerated alleles -> its `ploidy` alleles as VCF allele indices, ascending (the inverse
    of VCF genotype order: index = sum_i C(a_i + i - 1, i) over the sorted alleles a_1 <= ... <= a_K).  On a REFMASKED record the
    enumerated alleles start at the first alternate: every label is one higher."""
    from math import comb

    out, index = [], int(index)
    for i in range(int(ploidy), 0, -1):
        a = 0
        while comb(a + i, i) <= index:
            a += 1
        index -= comb(a + i - 1, i)
        out.append(a + (1 if refmasked else 0))
    return out[::-1]


# ---- record formatting (reference write_vcf_block and its helpers) ----------------------------------------------------
def vcf_sort_alleles(frequencies, reference_index):
    """Reference _vcf_sort_alleles: argsort(stable) reversed, the reference allele moved first."""
    frequencies = np.asarray(frequencies)
    n, a = frequencies.shape
    order = np.argsort(frequencies, axis=-1, kind="stable")[:, ::-1].astype(int)
    ref = np.asarray(reference_index)[:, None]
    alt = order.ravel()[(order != ref).ravel()].reshape(n, a - 1)
    return np.hstack([ref, alt])


def order_as_vcf_alleles(order, keep):
    """Reference _order_as_vcf_alleles: (REF strings, ALT strings) of ordered alleles, the alleles not kept left out."""
    chars = np.where(keep, ACGT[np.asarray(order)], "")
    ref = chars[:, 0]
    alts = np.array([",".join(c for c in row if c) for row in chars[:, 1:]], dtype="U7") if len(chars) else np.zeros(0, "U7")
    return ref, alts


def format_allele_counts(counts, keep, sep=","):
    """Reference format_allele_counts: per (variant, sample) the kept alleles' counts joined by `sep`."""
    counts = np.asarray(counts)
    n_variant, n_sample, n_allele = counts.shape
    keep = np.asarray(keep)
    if keep.ndim == 2:
        keep = keep[:, None, :]
    keep = np.broadcast_to(keep, counts.shape)
    chars = np.where(keep, counts.astype("U"), "")
    out = chars[:, :, 0]
    seps = np.where(keep, sep, "")
    for i in range(1, n_allele):
        out = np.char.add(np.char.add(out, seps[:, :, i]), chars[:, :, i])
    return out


def format_samples_columns(allele_depths, allele_keep):
    """Reference format_samples_columns without genotypes: [n, 1 + S] = the FORMAT column "GT:AD" and one ".:<AD>" per sample."""
    strings = np.char.add(".:", format_allele_counts(allele_depths, allele_keep))
    dt = "U%d" % max(5, strings.dtype.itemsize // 4)
    return np.concatenate([np.full((len(strings), 1), "GT:AD", dtype=dt), strings.astype(dt)], axis=1)


def format_genotype_columns(allele_depths, allele_keep, gt_index, gpm, ploidy, refmasked):
    """format_samples_columns with calls: [n, 1 + S] = the FORMAT column "GT:GPM:AD" and one "<GT>:<GPM>:<AD>" per sample.  GT:
    the mode's alleles as VCF indices, ascending, joined by "/" (`ploidy` dots for a no-call, gt_index < 0); GPM to 3 decimals."""
    gt_index, gpm = np.asarray(gt_index, dtype=np.int64), np.asarray(gpm, dtype=np.float64)
    n, S = gt_index.shape
    ploidy = np.broadcast_to(np.asarray(ploidy, dtype=np.int64), (S,))
    refmasked = np.asarray(refmasked, dtype=bool)
    gt = np.empty((n, S), dtype=object)
    for K in np.unique(ploidy):  # one table of genotype texts per (ploidy, masked): the last entry is the no-call
        cols = np.flatnonzero(ploidy == K)
        for masked in (False, True):
            rows = np.flatnonzero(refmasked == masked)
            if len(rows) == 0:
                continue
            g = gt_index[np.ix_(rows, cols)]
            table = np.array(["/".join(map(str, genotype_alleles(i, K, masked))) for i in range(int(g.max(initial=-1)) + 1)] +
                             ["/".join("." * int(K))], dtype=object)
            gt[np.ix_(rows, cols)] = table[np.where(g < 0, len(table) - 1, g)]
    values, inverse = np.unique(np.where(np.isnan(gpm), -1.0, gpm.round(3)), return_inverse=True)
    prob = np.array(["." if v < 0 else io.vcfstr(float(v)) for v in values], dtype=object)[inverse.reshape(n, S)]
    ad = format_allele_counts(allele_depths, allele_keep).astype(object)
    strings = gt + ":" + prob + ":" + ad
    return np.concatenate([np.full((n, 1), "GT:GPM:AD", dtype=object), strings], axis=1)


def format_records(contigs, positions, depth, flags, admf, gt_index=None, gpm=None, ploidy=None):
    """VCF record lines of the rows the filter kept: contigs / positions (0-based) per row, depth int [n, S, 4], flags [n],
    admf [n, 4] by allele index.  With gt_index / gpm [n, S] (genotypes_device's, of these rows) and ploidy (one value or one per
    sample) the sample columns are GT:GPM:AD instead of GT:AD with a null GT."""
    n = len(positions)
    if n == 0:
        return []
    _, keep, order, refmasked = decode_flags(flags)
    keep = np.take_along_axis(keep, order, axis=1)
    keep[:, 0] = True
    d = np.take_along_axis(np.asarray(depth, dtype=np.int64), order[:, None, :], axis=2)
    f = np.take_along_axis(np.asarray(admf, dtype=np.float64), order, axis=1).round(3)
    ref, alts = order_as_vcf_alleles(order, keep)
    pop = d.sum(axis=1)
    if gt_index is None:
        cols = format_samples_columns(d, keep)
    else:
        if gpm is None or ploidy is None:
            raise ValueError("format_records: gt_index needs gpm and ploidy")
        cols = format_genotype_columns(d, keep, gt_index, gpm, ploidy, refmasked)
    out = []
    for i in range(n):
        k = keep[i]
        info = "AD=" + io.vcfstr(pop[i][k]) + ";ADMF=" + io.vcfstr(f[i][k])
        if refmasked[i]:
            info = "REFMASKED;" + info
        out.append("\t".join([contigs[i], str(int(positions[i]) + 1), ".", ref[i], alts[i], ".", ".", info] + cols[i].tolist()))
    return out


# ---- the program ------------------------------------------------------------------------------------------------------
def plan_blocks(targets, max_rows):
    """Targets [(contig, start, stop)] in order -> blocks: lists of windows (contig, start, stop) on one contig, at most `max_rows`
    positions per block (a longer interval is split into windows)."""
    blocks, cur, rows = [], [], 0
    for contig, start, stop in targets:
        a = start
        while a < stop:
            if cur and (cur[-1][0] != contig or rows >= max_rows):
                blocks.append(cur)
                cur, rows = [], 0
            b = min(stop, a + max_rows - rows)
            cur.append((contig, a, b))
            rows += b - a
            a = b
    if cur:
        blocks.append(cur)
    return blocks


def block_rows_budget(n_samples):
    """Target positions per block: the depth tensor (16 B per sample) and the filter outputs within a share of the free HBM."""
    from .application import device_unit_budget

    return device_unit_budget(16 * n_samples + 48, fraction=0.25, least=TILE, most=1 << 20)


def find_snvs(targets, reference, source, maf=0.0, mad=0, ind_maf=0.1, ind_mad=3, min_ind=1, block_rows=None, tile=TILE, timings=None,
              genotypes=None):
    """Yield the VCF record lines of find-snvs: targets [(contig, start, stop)] (BED order; overlapping intervals are processed
    again), reference an io.Reference, source an application.ReadSource with one file per sample.  genotypes: None (GT:AD with a
    null GT), or the settings of genotypes_device as a dict (ploidy, and optionally inbreeding, frequencies, error_rate; ploidy and
    inbreeding one value, one per sample in the source's order, or a {sample: value} mapping): the records then carry GT:GPM:AD."""
    import torch

    lengths = dict(reference.contigs)
    for contig, start, stop in targets:
        if contig not in lengths:
            raise ValueError("target %s:%d-%d: contig %s is not in the reference" % (contig, start, stop, contig))
        if not 0 <= start < stop:
            raise ValueError("target %s:%d-%d: empty or negative interval" % (contig, start, stop))
        if stop > lengths[contig]:
            raise ValueError("target %s:%d-%d runs past the end of contig %s (length %d)" % (contig, start, stop, contig, lengths[contig]))
    files = _Files(source)
    S = len(files.samples)
    if genotypes is not None:
        genotypes = dict(genotypes)
        for key in ("ploidy", "inbreeding"):
            if isinstance(genotypes.get(key), dict):
                genotypes[key] = [genotypes[key][s] for s in files.samples]
        ploidy = genotypes["ploidy"]
    for block in plan_blocks(targets, int(block_rows or block_rows_budget(S))):
        depth, rows0 = _block_depths(files, block, tile=tile, timings=timings)
        ref = np.concatenate([bases_to_indices(reference.fetch(c, a, b).upper()) for c, a, b in block])
        ev = _events(timings)
        flags, admf = filter_device(depth, torch.from_numpy(ref), maf=maf, mad=mad, ind_maf=ind_maf, ind_mad=ind_mad, min_ind=min_ind)
        if genotypes is not None:
            eg = _events(timings)
            gt, gpm = genotypes_device(depth, flags, admf, **genotypes)
            if eg is not None:
                eg[1].record()
                timings["_events"].append(("genotypes", eg[0], eg[1]))
        idx = torch.nonzero(flags & 1).squeeze(1)
        kept_depth = depth.index_select(0, idx).cpu().numpy()
        calls = {} if genotypes is None else dict(gt_index=gt.index_select(0, idx).cpu().numpy(), gpm=gpm.index_select(0, idx).cpu().numpy(),
                                                  ploidy=ploidy)
        kept_flags, kept_admf, rows = flags.index_select(0, idx).cpu().numpy(), admf.index_select(0, idx).cpu().numpy(), idx.cpu().numpy()
        if ev is not None:
            ev[1].record()
            timings["_events"].append(("filter", ev[0], ev[1]))
        t0 = time.perf_counter()
        w = np.searchsorted(rows0, rows, side="right") - 1
        positions = np.array([b[1] for b in block], dtype=np.int64)[w] + (rows - rows0[w])
        lines = format_records([block[0][0]] * len(rows), positions, kept_depth, kept_flags, kept_admf, **calls)
        if timings is not None:
            timings["format"] = timings.get("format", 0.0) + time.perf_counter() - t0
            timings["records"] = timings.get("records", 0) + len(lines)
        yield from lines


def kernel_ms(timings):
    """Milliseconds of the timed launches so far by kind (HIP events; waits for them)."""
    out = {}
    for kind, e0, e1 in timings.get("_events", []):
        e1.synchronize()
        out[kind] = out.get(kind, 0.0) + e0.elapsed_time(e1)
    return out
