"""Plain per-read restatements of find-snvs (tests only): the pileup counting rule read by read, and the reference's
write_vcf_block filter in numpy.  mchap_amd/find_snvs.py and its kernels are held against these."""
import numpy as np

NIB = {"A": 0, "C": 1, "G": 2, "T": 3}


def _ref_span(cigar):
    return sum(n for n, op in cigar if op in "MDN=X")


def _aligned_positions(rec):
    """{reference position: read offset} of the M/=/X bases of a record dict (synth.write_bam form)."""
    out, ref, rd = {}, rec["pos"], 0
    for n, op in rec["cigar"]:
        if op in "M=X":
            for i in range(n):
                out[ref + i] = rd + i
        if op in "MDN=X":
            ref += n
        if op in "MIS=X":
            rd += n
    return out


def passes(rec, tid, min_quality=20, skip_duplicates=True, skip_qcfail=True, skip_supplementary=True):
    f = rec["flag"]
    if rec["ref"] != tid or f & 0x4 or f & 0x100 or rec["mapq"] < min_quality:
        return False
    if (skip_duplicates and f & 0x400) or (skip_qcfail and f & 0x200) or (skip_supplementary and f & 0x800):
        return False
    return not (f & 0x1 and not f & 0x2)  # orphan


def count(records, tid, start, stop, read_filter=None, min_bq=13):
    """int64 [stop - start, 4] allele depths of one sample's records (file order) over [start, stop) of reference tid."""
    kw = read_filter or {}
    recs = [dict(r, qual=list(r["qual"])) for r in records
            if passes(r, tid, **kw) and r["pos"] < stop and r["pos"] + _ref_span(r["cigar"]) > start]
    # htslib's overlap rule, record by record
    held = {}
    for r in recs:
        end = r["pos"] + _ref_span(r["cigar"])
        r["_end"] = end
        f = r["flag"]
        if not (f & 0x2) or f & 0x8 or r.get("next_ref", -1) != r["ref"]:
            continue
        a = held.get(r["qname"])
        if a is not None and r["pos"] >= a["_end"]:
            del held[r["qname"]]
            a = None
        if a is None:
            if r.get("next_pos", -1) >= r["pos"] or (f & 0x1 and r.get("next_pos", -1) == -1):
                held[r["qname"]] = r
            continue
        del held[r["qname"]]
        pa, pb = _aligned_positions(a), _aligned_positions(r)
        for p in sorted(set(pa) & set(pb)):
            i, j = pa[p], pb[p]
            qa, qb = a["qual"][i], r["qual"][j]
            if a["seq"][i] == r["seq"][j]:
                a["qual"][i], r["qual"][j] = min(qa + qb, 200), 0
            elif qa >= qb:
                a["qual"][i], r["qual"][j] = int(0.8 * qa) & 255, 0
            else:
                a["qual"][i], r["qual"][j] = 0, int(0.8 * qb) & 255
    out = np.zeros((stop - start, 4), dtype=np.int64)
    for r in recs:
        for p, i in _aligned_positions(r).items():
            if start <= p < stop and r["seq"][i] in NIB and r["qual"][i] >= min_bq:
                out[p - start, NIB[r["seq"][i]]] += 1
    return out


def write_vcf_block_filter(depth, ref_index, maf=0.0, mad=0, ind_maf=0.1, ind_mad=3, min_ind=1):
    """The reference's write_vcf_block steps on int depths [P, S, 4]: -> (kept rows, order [n, 4], keep [n, 4] in that order with
    the reference forced in, refmasked [n], ADMF [n, 4] in that order, unrounded)."""
    depth = np.asarray(depth, dtype=np.int64)
    ref_index = np.asarray(ref_index)
    rows = np.flatnonzero(ref_index >= 0)
    d, ri = depth[rows], ref_index[rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = d / d.sum(axis=-1, keepdims=True)
    keep = ((f >= ind_maf) & (d >= ind_mad)).sum(axis=1) >= min_ind
    if maf > 0.0:
        keep &= np.mean(f, axis=1) >= maf
    if mad > 0:
        keep &= np.sum(d, axis=1) >= mad
    idx = keep.sum(axis=-1) > 1
    rows, d, f, keep, ri = rows[idx], d[idx], f[idx], keep[idx], ri[idx]
    f = np.where(keep[:, None, :], f, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            admf = np.nanmean(f, axis=1)
    order = np.argsort(admf, axis=-1, kind="stable")[:, ::-1].astype(int)
    n = len(rows)
    alt = order.ravel()[(order != ri[:, None]).ravel()].reshape(n, 3)
    order = np.hstack([ri[:, None], alt])
    keep = np.take_along_axis(keep, order, axis=1)
    refmasked = ~keep[:, 0]
    keep[:, 0] = True
    return rows, order, keep, refmasked, np.take_along_axis(admf, order, axis=1)


def crafted_records(seed=7, n_single=260, n_pairs=90, length=700):
    """Records of one sample (synth.write_bam form, coordinate-sorted) on contigs c1 (`length`) and c2 (300) covering the
    counting rule's cases: base qualities 12 / 13 / 255, N and IUPAC bases, I / D / N / S operations, MAPQ, every flag with and
    without its --keep-* flag, secondary, unmapped, orphans, and proper pairs whose mates overlap (agreeing, disagreeing either
    way, equal qualities, odd qualities for the 0.8 truncation, a deletion inside the overlap)."""
    rng = np.random.default_rng(seed)
    cigars = [[(40, "M")], [(10, "S"), (30, "M")], [(15, "M"), (3, "I"), (22, "M")], [(18, "M"), (4, "D"), (22, "M")],
              [(12, "M"), (30, "N"), (28, "M")], [(20, "=") , (1, "X"), (19, "M")], [(35, "M"), (5, "S")]]
    flags = [0, 0, 0, 0, 16, 0x400, 0x200, 0x800, 0x100, 0x1, 0x1 | 0x20]

    def seq_qual(cigar):
        n = sum(k for k, op in cigar if op in "MIS=X")
        seq = "".join(rng.choice(list("ACGTACGTACGTNR"), size=n))
        qual = rng.choice([12, 13, 13, 20, 30, 37, 40, 41, 255], size=n).tolist()
        return seq, qual

    recs = []
    for i in range(n_single):
        cig = cigars[rng.integers(len(cigars))]
        seq, qual = seq_qual(cig)
        ref = 0 if rng.random() < 0.85 else 1
        pos = int(rng.integers(0, (length if ref == 0 else 300) - 80))
        recs.append(dict(qname="s%d" % i, flag=int(rng.choice(flags)), ref=ref, pos=pos, mapq=int(rng.choice([0, 19, 20, 25, 60])),
                         cigar=cig, seq=seq, qual=qual, rg="rg1"))
    recs.append(dict(qname="unmapped", flag=0x4, ref=0, pos=100, mapq=0, cigar=[(30, "M")], seq="A" * 30, qual=[30] * 30, rg="rg1"))
    for i in range(n_pairs):
        ca = [(40, "M")] if i % 5 else [(10, "M"), (3, "D"), (27, "M")]
        cb = [(40, "M")] if i % 7 else [(20, "M"), (2, "D"), (20, "M")]
        sa, qa = seq_qual(ca)
        sb, qb = seq_qual(cb)
        pa = int(rng.integers(0, length - 120))
        pb = pa + int(rng.integers(0, 45))
        kind = i % 4  # 0: mates agree where they overlap; 1: disagree; 2: copy with equal qualities; 3: as drawn
        la, lb = list(sa), list(sb)
        pos_a = _aligned_positions(dict(pos=pa, cigar=ca))
        pos_b = _aligned_positions(dict(pos=pb, cigar=cb))
        for p in set(pos_a) & set(pos_b):
            i_a, i_b = pos_a[p], pos_b[p]
            if kind in (0, 2):
                lb[i_b] = la[i_a]
            elif kind == 1:
                lb[i_b] = "ACGT"[("ACGT".index(la[i_a]) + 1) % 4] if la[i_a] in "ACGT" else "A"
            if kind == 2:
                qb[i_b] = qa[i_a]
        fl = 0x1 | 0x2 | (0x40 if i % 2 else 0x80)
        if i % 11 == 0:
            fl |= 0x8  # mate unmapped: no overlap rule
        recs.append(dict(qname="p%d" % i, flag=fl, ref=0, pos=pa, mapq=60, cigar=ca, seq="".join(la), qual=qa, rg="rg1",
                         next_ref=0, next_pos=pb, tlen=pb + 40 - pa))
        recs.append(dict(qname="p%d" % i, flag=0x1 | 0x2 | (0x80 if i % 2 else 0x40), ref=0, pos=pb, mapq=60, cigar=cb, seq="".join(lb),
                         qual=qb, rg="rg1", next_ref=0, next_pos=pa, tlen=-(pb + 40 - pa)))
    recs.sort(key=lambda r: (r["ref"], r["pos"]))
    return [("c1", length), ("c2", 300)], recs
