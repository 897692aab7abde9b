"""VCF record lines of the three programs from their per-sample results (application/baseclass.py:220-302, call_exact.py:84-199,
assemble.py:144-305, assemble/haplotype_calling.py:4-64): `call` and `call-exact` share _format_exact_record; `assemble` has the
per-locus formatter _assemble_record_line (the definition) and _block_record_line, the same line from the summary arrays of a block."""
import numpy as np

from .io import qual_of_prob, vcfstr


SAMPLE_FIELDS = ("GT", "GQ", "SQ", "DP", "RCOUNT", "RCALLS", "MEC", "MECP", "GPM", "SPM", "MCI")


def _mec(calls, genotype):
    """minimum_error_correction summed over reads (encoding/integer/stats.py:18-39)."""
    if len(calls) == 0:
        return 0
    diff = (calls[:, None, :] != genotype[None]) & (calls[:, None, :] >= 0)
    return int(diff.sum(axis=-1).min(axis=-1).sum())


def _rounded_text(r):
    """io._number_text of a value already rounded by np.round (an array's worth at a time)."""
    if r != r:
        return "."
    if abs(r) != float("inf") and r == int(r):
        return str(int(r))
    return repr(r)[:16]


def _format_exact_record(unit, samples, results, ri, ploidy_of, report, prior_tag):
    """(FILTER, INFO, FORMAT, {sample: column}) of one record from the units' results (application/baseclass.py:220-302,
    call_exact.py:84-199).  A result with an "mci" (the sampler of `call`; the exact caller has none) puts it into the sample's
    MCI field, and INFO MCI counts the samples where it is above 0."""
    from .vcfheader import report_fields

    info_opt, fmt_opt = report_fields(report)
    rec, locus, invalid = unit["rec"], unit["locus"], unit["invalid"]
    haps = locus.haplotypes
    H, M = haps.shape
    cols, gts = {}, {}
    acp_sum = np.zeros(H)
    aop_not = np.ones(H)
    aop_sum = np.zeros(H)
    snvdp_sum = np.zeros(M)
    dps, rcounts = [], []
    nan_arrays = False
    ploidy_total = 0
    n_mci = 0
    for sample in samples:
        ploidy = int(ploidy_of(sample))
        ploidy_total += ploidy
        sr = unit["reads"][sample]
        calls, depth = sr["calls"], sr["depth"]
        rcount = len(calls)
        dp = np.round(np.mean(depth)) if len(depth) else np.nan
        rcalls = int((calls >= 0).sum())
        dps.append(dp)
        rcounts.append(rcount)
        if M:
            snvdp_sum += np.round(depth)
        if invalid:
            gts[sample] = np.full(ploidy, -1, int)
            fields = ["/".join(["."] * ploidy), ".", ".", vcfstr(float(dp)), str(rcount), str(rcalls), ".", ".", ".", ".", "."]
            fields += ["."] * len(fmt_opt)
            cols[sample] = ":".join(fields)
            nan_arrays = True
            continue
        res = results.get((ri, sample)) if (M == 0 or H == 1) else results[(ri, sample)]
        mci = None if res is None else res.get("mci")
        n_mci += int(mci is not None and mci > 0)
        if M == 0 or H == 1:
            # a single haplotype: one genotype with probability 1 (the reference's arithmetic gives exactly that)
            res = dict(alleles=np.zeros(ploidy, int), gprob=1.0, sprob=1.0, freqs=np.ones(1), occur=np.ones(1), GL=np.zeros(1), GP=np.ones(1))
        alleles = np.asarray(res["alleles"])
        gprob, sprob = res["gprob"], res["sprob"]
        gts[sample] = alleles
        freqs, occur = np.asarray(res["freqs"], float), np.asarray(res["occur"], float)
        acp_sum += freqs * ploidy
        aop_sum += occur
        aop_not *= 1 - occur
        mec = _mec(calls, haps[alleles])
        denom = int((calls >= 0).sum())
        mecp = mec / denom if denom > 0 else np.nan
        fields = ["/".join(str(a) for a in alleles), vcfstr(qual_of_prob(gprob)), vcfstr(qual_of_prob(sprob)), vcfstr(float(dp)),
                  str(rcount), str(rcalls), str(mec), vcfstr(float(mecp)), vcfstr(float(gprob)), vcfstr(float(sprob)),
                  "." if mci is None else str(mci)]
        for tag in fmt_opt:
            if tag == "AFP":
                fields.append(vcfstr(freqs))
            elif tag == "ACP":
                fields.append(vcfstr(freqs * ploidy))
            elif tag == "AOP":
                fields.append(vcfstr(occur))
            elif tag == "SNVDP":
                fields.append(vcfstr(np.round(depth).astype(float)) if len(depth) else ".")
            elif tag in ("GL", "GP"):
                fields.append(vcfstr(np.asarray(res[tag], float)))
        cols[sample] = ":".join(fields)
    # ---- record level ----
    counts = np.zeros(H, int)
    for g in gts.values():
        for a in g:
            if a >= 0:
                counts[a] += 1
    info = [("AN", int(counts.sum())), ("UAN", int((counts > 0).sum())), ("AC", counts[1:])]
    if locus.mask_reference_allele:
        info.append(("REFMASKED", True))
    info += [("NS", sum(int(np.any(g >= 0)) for g in gts.values())), ("MCI", n_mci),
             ("DP", float(np.nansum(dps)) if M else np.nan), ("RCOUNT", int(np.nansum(rcounts))), ("END", locus.stop),
             ("NVAR", M), ("SNVPOS", np.array(locus.positions, int) - locus.start + 1)]
    null_r = np.full(H, np.nan)
    for tag in info_opt:
        if tag == "AFPRIOR":
            info.append(("AFPRIOR", locus.frequencies))
        elif tag == "ACP":
            info.append(("ACP", null_r if nan_arrays else acp_sum))
        elif tag == "AFP":
            info.append(("AFP", null_r if nan_arrays else acp_sum / ploidy_total))
        elif tag == "AOP":
            info.append(("AOP", null_r if nan_arrays else 1 - aop_not))
        elif tag == "AOPSUM":
            info.append(("AOPSUM", null_r if nan_arrays else aop_sum))
        elif tag == "SNVDP":
            info.append(("SNVDP", snvdp_sum))
    parts = []
    for k, v in info:
        if isinstance(v, bool):
            if v:
                parts.append(k)
        else:
            parts.append("%s=%s" % (k, vcfstr(np.asarray(v) if isinstance(v, np.ndarray) else v)))
    if "emit" in unit:   # (call-exact --estimate-prior-frequencies: the iterations run for the record, null where none was)
        parts.append("EMIT=%s" % ("." if unit["emit"] is None or invalid else unit["emit"]))
    fmt = ":".join(SAMPLE_FIELDS + tuple(fmt_opt))
    return invalid or "PASS", ";".join(parts), fmt, cols


def call_posterior_haplotypes(posteriors, threshold=0.01):
    """The haplotype alleles of a VCF record from the samples' posteriors (same name and result as the reference's
    assemble/haplotype_calling.py): a haplotype is listed when its posterior probability of occurrence reaches
    `threshold` in at least one sample; listed haplotypes are ranked by their expected dosage summed over the samples
    that list them, the all-reference haplotype always first.  Returns (haplotypes int8 [n, n_base], ref_observed)."""
    from .classes import _first_occurrence_unique

    n_base = posteriors[0].genotypes.shape[-1]
    rows, weights = [], []
    for post in posteriors:
        haps, dosage, occurrence = post.allele_frequencies(dosage=True)
        listed = occurrence >= threshold
        rows.append(np.asarray(haps[listed], dtype=np.int8).reshape(int(np.sum(listed)), n_base))
        weights.append(dosage[listed])
    rows = np.concatenate(rows) if rows else np.zeros((0, n_base), np.int8)
    weights = np.concatenate(weights) if weights else np.zeros(0)
    if len(rows):
        first, ids = _first_occurrence_unique(rows)      # distinct haplotypes in order of first listing
        distinct = rows[first]
        score = np.zeros(len(distinct))
        np.add.at(score, ids, weights)                   # summed sample after sample
    else:
        distinct, score = rows, np.zeros(0)
    is_ref = (distinct == 0).all(axis=1) if len(distinct) else np.zeros(0, bool)
    ref_observed = bool(is_ref.any())
    distinct, score = distinct[~is_ref], score[~is_ref]
    haplotypes = np.concatenate([distinct, np.zeros((1, n_base), np.int8)]).astype(np.int8)
    value = np.append(score, (score.max() if len(score) else -1.0) + 1.0)  # the reference allele outranks everything
    return haplotypes[np.flip(np.argsort(value))], ref_observed


def _genotype_posterior_array(post, labels, ploidy):
    """Posterior probabilities of all genotypes over the record's labelled alleles, in VCF order (application/assemble.py:
    276-305): a posterior genotype that holds an allele the record does not list cannot be encoded and is left out."""
    from math import comb

    from .calling_mcmc import _vcf_index

    # (every allele of the record counts, a masked reference allele included: Number=G.  The reference sizes the array by
    # len(labels), one short when the reference allele is masked, and then fails with an IndexError on the last allele.)
    n_alleles = max(labels.values()) + 1 if labels else 1
    out = np.zeros(comb(n_alleles + ploidy - 1, ploidy), float)
    for haps, prob in zip(post.genotypes, post.probabilities):
        alleles = np.sort([labels.get(np.asarray(h, dtype=np.int8).tobytes(), -1) for h in haps])
        if alleles[0] >= 0:
            out[int(_vcf_index(alleles[None])[0])] = prob
    return out


def _no_snv_result(ploidy):
    """The sampler's summary of a unit without SNVs: nothing is sampled, the empty genotype has probability 1."""
    return dict(genotypes=np.zeros((1, ploidy, 0), np.int8), probabilities=np.ones(1), spm=1.0, gpm=1.0,
                mode_genotype=np.zeros((ploidy, 0), np.int8), mci=0)


def _sample_summary(res, calls, depth):
    """per[sample] of _assemble_record_line from a unit's posterior summary and its reads' calls and depth."""
    mec = _mec(calls, res["mode_genotype"])
    denom = int((calls >= 0).sum())
    return dict(genotype=res["mode_genotype"], gprob=float(res["gpm"]), sprob=float(res["spm"]), mec=mec,
                mecp=mec / denom if denom > 0 else np.nan, mci=int(res["mci"]), rcount=len(calls), rcalls=denom,
                dp=np.round(np.mean(depth)) if len(depth) else np.nan, depth=depth)


def _limit_record_line(locus, samples, report=(), ploidy_of=None):
    """The record of a target the library could not sample (beyond its shape limits: the reference has none, so this is a gap
    of this build, made visible): REF, no ALT, FILTER = LIMIT, the INFO fields that do not depend on the sampler, and null
    genotypes of each sample's ploidy -- never an omitted record (an incomplete file is worse than a flagged one)."""
    from .vcfheader import report_fields

    _, fmt_opt = report_fields(report)
    M = len(locus.positions)
    info = "AN=0;UAN=0;AC=.;NS=0;MCI=0;DP=.;RCOUNT=.;END=%d;NVAR=%d;SNVPOS=%s" % (
        locus.stop, M, vcfstr(np.array(locus.positions, int) - locus.start + 1))
    cols = []
    for sample in samples:
        K = int(ploidy_of(sample)) if ploidy_of is not None else 2
        cols.append(":".join(["/".join(["."] * K)] + ["."] * (len(SAMPLE_FIELDS) - 1 + len(fmt_opt))))
    return "\t".join([locus.contig, str(locus.start + 1), locus.name, locus.sequence, ".", ".", "LIMIT", info,
                      ":".join(SAMPLE_FIELDS + tuple(fmt_opt))] + cols)


def _assemble_record_line(locus, samples, per, posteriors, haplotype_posterior_threshold, report=(), ploidy_of=None, encoded=None):
    """The VCF record line of `mchap assemble` from the per-sample summaries (application/assemble.py:144-252,
    baseclass.py:220-302).  per[sample]: genotype [K, M], gprob, sprob, mec, mecp, mci, rcount, rcalls, dp, depth;
    encoded[sample]: the sample's encoded reads (for --report GL)."""
    from .vcfheader import report_fields

    info_opt, fmt_opt = report_fields(report)
    M = len(locus.positions)
    haplotypes, ref_called = call_posterior_haplotypes(posteriors, threshold=haplotype_posterior_threshold)
    labels = {h.tobytes(): i for i, h in enumerate(haplotypes)}
    flt = "PASS"
    if not ref_called:
        labels.pop(haplotypes[0].tobytes())
        if len(haplotypes) == 1:
            flt = "NOA"
    H = len(haplotypes)
    alts = [locus.format_haplotype(h) for h in haplotypes[1:]]
    counts = np.zeros(H, int)
    cols = []
    want_afp = bool({"ACP", "AFP", "AOP", "AOPSUM"} & set(info_opt)) or bool({"ACP", "AFP", "AOP"} & set(fmt_opt))
    acp_sum, aop_sum, aop_not, snvdp_sum = np.zeros(H), np.zeros(H), np.ones(H), np.zeros(M)
    ploidy_total = 0
    for sample, post in zip(samples, posteriors):
        d = per[sample]
        K = len(d["genotype"])
        ploidy_total += K
        a = np.sort([labels.get(np.asarray(h, dtype=np.int8).tobytes(), -1) for h in d["genotype"]])
        a = np.append(a[a >= 0], a[a < 0])
        for x in a:
            if x >= 0:
                counts[x] += 1
        d["alleles"] = a
        fields = ["/".join(str(x) if x >= 0 else "." for x in a), vcfstr(qual_of_prob(d["gprob"])), vcfstr(qual_of_prob(d["sprob"])),
                  vcfstr(float(d["dp"])), str(d["rcount"]), str(d["rcalls"]), str(d["mec"]), vcfstr(float(d["mecp"])),
                  vcfstr(d["gprob"]), vcfstr(d["sprob"]), str(d["mci"])]
        depth = np.asarray(d.get("depth", np.zeros(M)), float)
        if M:
            snvdp_sum += np.round(depth)
        freqs = occur = None
        if want_afp:
            # posterior allele frequencies / occurrences of the record's haplotypes (assemble.py:213-226)
            freqs, occur = np.zeros(H), np.zeros(H)
            hp, fq, oc = post.allele_frequencies()
            index = {np.asarray(h, dtype=np.int8).tobytes(): i for i, h in enumerate(haplotypes)}
            for h, f_, o_ in zip(hp, fq, oc):
                i = index.get(np.asarray(h, dtype=np.int8).tobytes())
                if i is not None:
                    freqs[i], occur[i] = f_, o_
            acp_sum += freqs * K
            aop_sum += occur
            aop_not *= 1 - occur
        for tag in fmt_opt:
            if tag == "AFP":
                fields.append(vcfstr(freqs))
            elif tag == "ACP":
                fields.append(vcfstr(freqs * K))
            elif tag == "AOP":
                fields.append(vcfstr(occur))
            elif tag == "GP":
                fields.append(vcfstr(_genotype_posterior_array(post, labels, K)))
            elif tag == "GL":
                # likelihoods of every genotype over the record's haplotypes (assemble.py:236-244): the exact caller's kernel
                from . import calling

                sr = encoded[sample]
                if M and len(sr["dists"]):
                    llks = calling.genotype_likelihoods(sr["dists"], K, haplotypes, read_counts=sr["counts"])
                else:
                    from math import comb

                    llks = np.zeros(comb(H + K - 1, K), np.float32)
                fields.append(vcfstr(np.asarray(llks, np.float64) / np.log(10)))
            elif tag == "SNVDP":
                fields.append(vcfstr(np.round(depth)) if M else ".")
        cols.append(":".join(fields))
    info = [("AN", int(counts.sum())), ("UAN", int((counts > 0).sum())), ("AC", counts[1:])]
    if not ref_called:
        info.append(("REFMASKED", True))
    info += [("NS", sum(int(np.any(per[s]["alleles"] >= 0)) for s in samples)), ("MCI", sum(int(per[s]["mci"] > 0) for s in samples)),
             ("DP", float(np.nansum([per[s]["dp"] for s in samples])) if M else np.nan),
             ("RCOUNT", int(sum(per[s]["rcount"] for s in samples))), ("END", locus.stop), ("NVAR", M),
             ("SNVPOS", np.array(locus.positions, int) - locus.start + 1)]
    for tag in info_opt:
        if tag == "AFPRIOR":
            info.append(("AFPRIOR", np.full(H, np.nan)))  # (the assembler has no prior allele frequencies)
        elif tag == "ACP":
            info.append(("ACP", acp_sum))
        elif tag == "AFP":
            info.append(("AFP", acp_sum / ploidy_total))
        elif tag == "AOP":
            info.append(("AOP", 1 - aop_not))
        elif tag == "AOPSUM":
            info.append(("AOPSUM", aop_sum))
        elif tag == "SNVDP":
            info.append(("SNVDP", snvdp_sum))
    parts = []
    for k, v in info:
        if isinstance(v, bool):
            if v:
                parts.append(k)
        else:
            parts.append("%s=%s" % (k, vcfstr(v)))
    return "\t".join([locus.contig, str(locus.start + 1), locus.name, locus.sequence, ",".join(alts) if alts else ".", ".", flt,
                      ";".join(parts), ":".join(SAMPLE_FIELDS + tuple(fmt_opt))] + cols)


_FMT_HEAD = ":".join(SAMPLE_FIELDS)


def _block_record_line(locus, xi, M, sums, at, encs, K_of, mec_of, mecp_of):
    """_assemble_record_line without --report fields, from the summary arrays of a block (application._BlockState._summaries) and
    never through PosteriorGenotypeDistribution objects: the fast formatter of the block path.  xi: the locus among the block's
    encoded loci, M its SNVs; at [S, 2]: per sample (index into `sums`, unit within that batch); encs: the samples' block encodings;
    K_of: their ploidies; mec_of [S, loci], mecp_of [S][loci]: MEC and rounded MECP of every unit."""
    S = len(K_of)
    at = at.tolist()
    # call_posterior_haplotypes: the haplotypes any sample lists, ranked by expected dosage summed over the samples
    index, score = {}, []
    for si in range(S):
        sm, u = sums[at[si][0]], at[si][1]
        B, cell_of, lw = sm["B"], sm["cell_of"], sm["lweight"]
        for k in range(int(sm["lstart"][u]), int(sm["lstart"][u + 1])):
            c0 = int(cell_of[k])
            key = B[c0:c0 + M]
            i = index.get(key)
            if i is None:
                index[key] = len(score)
                score.append(0.0 + lw[k])
            else:
                score[i] += lw[k]
    ref = bytes(M)
    ref_called = ref in index
    keys = [k_ for k_ in index if k_ != ref]
    vals = [score[index[k_]] for k_ in keys]
    keys.append(ref)
    vals.append((max(vals) if vals else -1.0) + 1.0)
    if len(keys) > 2:
        if len(set(vals)) == len(vals):   # (no ties: the descending order is unique)
            keys = [keys[i] for i in sorted(range(len(vals)), key=vals.__getitem__, reverse=True)]
        else:
            keys = [keys[i] for i in np.flip(np.argsort(np.array(vals))).tolist()]
    elif len(keys) == 2:
        keys = [keys[1], keys[0]]
    labels = {k_: i for i, k_ in enumerate(keys)}
    flt = "PASS"
    if not ref_called:
        labels.pop(ref)
        if len(keys) == 1:
            flt = "NOA"
    H = len(keys)
    seq0 = list(locus.sequence)
    alts = []
    rel = [p_ - locus.start for p_ in locus.positions]
    for key in keys[1:]:
        chars = seq0[:]
        for r_, tup, a in zip(rel, locus.alleles, key):
            chars[r_] = tup[a]
        alts.append("".join(chars))
    counts = [0] * H
    cols, ns, n_mci, dp_sum, rc_sum = [], 0, 0, 0.0, 0
    for si in range(S):
        sm, u = sums[at[si][0]], at[si][1]
        K = K_of[si]
        enc = encs[si]
        m0 = int(sm["mode_slot"][u])
        cell_of, B = sm["cell_of"], sm["B"]
        a = []
        for h in range(K):
            c0 = int(cell_of[m0 + h])
            a.append(labels.get(B[c0:c0 + M], -1))
        a.sort()
        neg = [x for x in a if x < 0]
        a = [x for x in a if x >= 0]
        for x in a:
            counts[x] += 1
        if a:
            ns += 1
        mci = int(sm["mci"][u])
        n_mci += mci > 0
        mec = int(mec_of[si, xi])
        rcalls, rcount, dp = int(enc.rcalls[xi]), int(enc.rcount[xi]), float(enc.dp[xi])
        if dp == dp:
            dp_sum += dp
        rc_sum += rcount
        mecp = _rounded_text(mecp_of[si][xi]) if rcalls > 0 else "."
        cols.append(":".join(["/".join([str(x) for x in a] + ["."] * len(neg)), str(int(sm["gq"][u])), str(int(sm["sq"][u])),
                              _rounded_text(dp), str(rcount), str(rcalls), str(mec), mecp,
                              _rounded_text(sm["gpm"][u]), _rounded_text(sm["spm"][u]), str(mci)]))
    info = ["AN=%d" % sum(counts), "UAN=%d" % sum(1 for x in counts if x > 0), "AC=" + (",".join(str(x) for x in counts[1:]) if H > 1 else ".")]
    if not ref_called:
        info.append("REFMASKED")
    info += ["NS=%d" % ns, "MCI=%d" % n_mci, "DP=" + _rounded_text(dp_sum), "RCOUNT=%d" % rc_sum, "END=%d" % locus.stop,
             "NVAR=%d" % M, "SNVPOS=" + ",".join(str(r_ + 1) for r_ in rel)]
    return "\t".join([locus.contig, str(locus.start + 1), locus.name, locus.sequence, ",".join(alts) if alts else ".", ".", flt,
                      ";".join(info), _FMT_HEAD] + cols)
