"""`mchap atomize` (reference application/atomize.py): a VCF of haplotype calls split into one record per basis SNV, with the
sample fields GT:GQ:PQ:DP:DS -- how haplotype calls reach tools that only read SNVs.  Host only.  The projection of a haplotype
record onto its SNVs and the text of the SNV records are here once: the program `atomize` and the SNV file `call-exact
--snv-calls` writes during its run (application.SnvCalls) both go through snv_block_lines, the second with GQ, DS and ACP (and GP)
taken from the exact SNV genotype posteriors instead of the record's own fields.

No pysam, no pandas: the records come from io.read_vcf."""
from datetime import date
from math import comb

import numpy as np

from .io import open_text, read_vcf

# (id, Number, Type, Description) of the SNV file's header, in the order written (reference atomize.py:255-271)
SNV_INFO_FIELDS = [
    ("AC", "A", "Integer", "Allele count in genotypes, for each ALT allele, in the same order as listed"),
    ("ACP", "R", "Float", "Posterior allele counts"),
    ("DP", "1", "Integer", "Combined depth across samples"),
    ("PS", "1", "Integer", "Phased set for all samples"),
]
SNV_FORMAT_FIELDS = [
    ("GT", "1", "String", "Genotype"),
    ("GQ", "1", "Integer", "Genotype quality"),
    ("PQ", "1", "Integer", "Phasing quality"),
    ("DP", "1", "Integer", "Read depth"),
    ("DS", "A", "Float", "Posterior mean dosage"),
]
SNV_GP_FIELD = ("GP", "G", "Float", "Genotype posterior probabilities")   # call-exact --snv-report GP only
MAX_SNV_ALLELES = 4   # the bases


def haplotype_snvs(rec):
    """chars [H, M]: the base of every haplotype (REF first, then the ALTs) at every position of INFO/SNVPOS; None when the record
    has no SNV (SNVPOS missing or '.')."""
    text = rec["info"].get("SNVPOS")
    if text in (None, True, ".", ""):
        return None
    pos = np.array([int(x) for x in str(text).split(",")]) - 1
    return np.array([[seq[p] for p in pos] for seq in (rec["ref"],) + tuple(rec["alts"])], dtype="U1").reshape(1 + len(rec["alts"]), len(pos))


def snv_allele_indices(snvs):
    """int [H, M]: at every SNV the allele index of every haplotype, in order of first appearance over the haplotypes (reference
    get_haplotype_snv_indices): haplotype 0 is REF, so index 0 is the reference base."""
    snvs = np.asarray(snvs)
    out = np.zeros(snvs.shape, dtype=int)
    for j in range(snvs.shape[1]):
        seen = {}
        for h in range(snvs.shape[0]):
            out[h, j] = seen.setdefault(snvs[h, j], len(seen))
    return out


def format_snv_alleles(snvs):
    """(REF chars [M], ALT texts [M], number of ALTs [M]) (reference format_snv_alleles): an SNV at which no haplotype differs from
    REF has the empty ALT ''."""
    snvs = np.asarray(snvs)
    idx = snv_allele_indices(snvs)
    alts, n_alts = [], []
    for j in range(snvs.shape[1]):
        first = [int(np.flatnonzero(idx[:, j] == a)[0]) for a in range(1, int(idx[:, j].max()) + 1)]
        alts.append(",".join(snvs[h, j] for h in first))
        n_alts.append(len(first))
    return snvs[0], np.array(alts, dtype="U"), np.array(n_alts, dtype=int)


def float_text(x, precision=3):
    """One float as the reference's format_allele_floats writes it: rounded, trailing zeros and a trailing point dropped, '.'
    for NaN."""
    if np.isnan(x):
        return "."
    return repr(float(np.round(float(x), precision))).rstrip("0").rstrip(".")


def format_allele_floats(array, alts_number, length="R", precision=3):
    """The comma-separated texts of per-allele floats [M, alleles] or [M, samples, alleles], cut to each SNV's number of ALT
    alleles (length 'A') or of all alleles ('R') (reference format_allele_floats)."""
    array = np.asarray(array, dtype=float)
    assert length in ("R", "A")
    if array.ndim not in (2, 3):
        raise ValueError("Number of dimensions not supported.")
    rows = []
    for limit, values in zip(alts_number, array):
        n = int(limit) + (1 if length == "R" else 0)
        if array.ndim == 2:
            rows.append(",".join(float_text(v, precision) for v in values[:n]))
        else:
            rows.append([",".join(float_text(v, precision) for v in sample[:n]) for sample in values])
    return np.array(rows, dtype="U")


def genotype_rank(alleles):
    """Rank in VCF order of the genotype with these alleles (any order)."""
    return sum(comb(int(a) + i, i + 1) for i, a in enumerate(sorted(int(a) for a in alleles)))


def _sample_field(rec, sample, tag):
    """The text of a FORMAT field of a sample, None when the record or the sample does not have it."""
    tags = rec["format"].split(":") if rec["format"] else []
    if tag not in tags:
        return None
    values = rec["samples"][sample].split(":")
    i = tags.index(tag)
    return values[i] if i < len(values) else None


def _floats(text):
    return np.array([np.nan if x in (".", "") else float(x) for x in text.split(",")])


def record_genotypes(rec, samples):
    """{sample: [allele or None, ...]} of FORMAT/GT ('/' or '|' separated)."""
    out = {}
    for s in samples:
        gt = _sample_field(rec, s, "GT") or "."
        out[s] = [None if a in (".", "") else int(a) for a in gt.replace("|", "/").split("/")]
    return out


def record_snv_counts(rec, samples, idx, ploidies):
    """float [M, samples, 4]: the samples' posterior allele counts of the record's own FORMAT/ACP -- else FORMAT/AFP times the
    ploidy -- added up by SNV allele and normalised to the ploidy (reference get_sample_snv_ACP); NaN for a sample with neither."""
    H, M = idx.shape
    out = np.zeros((M, len(samples), MAX_SNV_ALLELES))
    for i, s in enumerate(samples):
        text = _sample_field(rec, s, "ACP")
        if text is not None:
            counts = _floats(text)
        else:
            text = _sample_field(rec, s, "AFP")
            if text is None:
                out[:, i, :] = np.nan
                continue
            counts = _floats(text) * ploidies[i]
        for h, c in enumerate(counts[:H]):
            for p in range(M):
                out[p, i, idx[h, p]] += c
    denom = np.sum(out, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = out / np.where(denom == 0.0, np.nan, denom)
    return out * np.asarray(ploidies, dtype=float)[None, :, None]


def snv_block_lines(rec, samples, posterior=None):
    """The SNV record lines of one haplotype record (reference format_vcf_snv_block); [] for a record without SNVs.
    posterior: None (`atomize`: GQ '.', DS / ACP from the record's own ACP or AFP), or what the exact SNV posteriors give:
    dict(gq=texts [M][samples], counts=float [M, samples, 4] expected SNV allele counts (NaN: none), gp=texts [M][samples] or None)."""
    snvs = haplotype_snvs(rec)
    if snvs is None:
        return []
    idx = snv_allele_indices(snvs)
    H, M = idx.shape
    refs, alts, n_alts = format_snv_alleles(snvs)
    snvpos = np.array([int(x) for x in str(rec["info"]["SNVPOS"]).split(",")])
    gts = record_genotypes(rec, samples)
    ploidies = [len(gts[s]) for s in samples]
    hap_counts = np.zeros(H)
    gt_text = []
    for s in samples:
        calls = np.full((len(gts[s]), M), -1, dtype=int)
        for k, a in enumerate(gts[s]):
            if a is not None:
                hap_counts[a] += 1
                calls[k] = idx[a]
        gt_text.append(["|".join(str(a) if a >= 0 else "." for a in calls[:, j]) for j in range(M)])
    snv_counts = np.zeros((M, int(idx.max()) + 1))
    for h, c in enumerate(hap_counts):
        for j in range(M):
            snv_counts[j, idx[h, j]] += c
    counts = record_snv_counts(rec, samples, idx, ploidies) if posterior is None else np.asarray(posterior["counts"], dtype=float)
    ds = format_allele_floats(counts[:, :, 1:], n_alts, length="A") if len(samples) else np.zeros((M, 0), dtype="U")
    # PQ: the call's SQ as written ('.' for a null call: the reference would write Python's 'None' there -- DESIGN.md, quirks)
    pq = [_sample_field(rec, s, "SQ") or "." for s in samples]
    # DP: FORMAT/SNVDP; whole numbers while every sample has them, else the reference's float texts ('12.0') and '.' for a gap
    depth = np.full((M, len(samples)), np.nan)
    for i, s in enumerate(samples):
        text = _sample_field(rec, s, "SNVDP")
        if text is not None:
            d = _floats(text)
            if len(d) == M:
                depth[:, i] = d
    whole = bool(len(samples)) and not np.any(np.isnan(depth))
    dp_text = lambda v: "." if np.isnan(v) else (str(int(v)) if whole else repr(float(v)))
    ac = format_allele_floats(snv_counts[:, 1:], n_alts, length="A")
    acp = format_allele_floats(counts.sum(axis=1), n_alts, length="R")
    fmt = "GT:GQ:PQ:DP:DS" + (":GP" if posterior is not None and posterior.get("gp") is not None else "")
    rec_id = rec.get("id")
    lines = []
    for j in range(M):
        info = "AC=%s;ACP=%s;DP=%s;PS=%d" % (ac[j], acp[j], dp_text(depth[j].sum()) if len(samples) else ".", rec["pos"])
        cols = []
        for i in range(len(samples)):
            fields = [gt_text[i][j], "." if posterior is None else posterior["gq"][j][i], pq[i], dp_text(depth[j, i]), ds[j][i]]
            if fmt.endswith(":GP"):
                fields.append(posterior["gp"][j][i])
            cols.append(":".join(fields))
        lines.append("\t".join([rec["chrom"], str(int(snvpos[j]) - 1 + rec["pos"]),
                                "%s_SNV%d" % (rec_id, j + 1) if rec_id and rec_id != "." else ".", str(refs[j]), str(alts[j]), ".", ".",
                                info, fmt] + cols))
    return lines


def snv_header_lines(contig_lines, samples, command, gp=False, today=None, version=None):
    """The header of the SNV file (reference atomize_vcf:244-277).  contig_lines: the input's ##contig lines as they stand."""
    from . import __version__

    d = today or date.today()
    cmd = command if isinstance(command, str) else '"%s"' % " ".join(command)
    out = ["##fileformat=VCFv4.3", "##fileDate=%04d%02d%02d" % (d.year, d.month, d.day),
           "##source=mchap_amd v%s (atomize)" % (version or __version__), "##commandline=%s" % cmd]
    out += list(contig_lines)
    out += ['##INFO=<ID=%s,Number=%s,Type=%s,Description="%s">' % f for f in SNV_INFO_FIELDS]
    out += ['##FORMAT=<ID=%s,Number=%s,Type=%s,Description="%s">' % f for f in SNV_FORMAT_FIELDS + ([SNV_GP_FIELD] if gp else [])]
    out.append("#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + list(samples)))
    return out


def vcf_contig_lines(path):
    out = []
    with open_text(path) as f:
        for line in f:
            if not line.startswith("##"):
                break
            if line.startswith("##contig="):
                out.append(line.rstrip("\n"))
    return out


def atomize_vcf(path, out, command=None):
    """`atomize --haplotypes path`: the SNV file of a haplotype VCF (plain or gzip / bgzip compressed) written to `out`.  Returns
    the number of SNV records."""
    samples, records = read_vcf(path)
    for line in snv_header_lines(vcf_contig_lines(path), samples, command or "atomize %s" % path):
        out.write(line + "\n")
    n = 0
    for rec in records:
        for line in snv_block_lines(rec, samples):
            out.write(line + "\n")
            n += 1
    return n
