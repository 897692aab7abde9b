"""Command line of the programs built on the kernels: `python -m mchap_amd {assemble,call,call-exact,find-snvs,atomize} ...` with the
reference's flag names, defaults and meaning (application/cli.py:14-60; application/arguments.py: the argument tables
ASSEMBLE_MCMC_PARSER_ARGUMENTS / CALL_EXACT_PARSER_ARGUMENTS / CALL_MCMC_PARSER_ARGUMENTS and the collect_* functions)
for these three programs: every flag those tables define is accepted here with the same arity and default.  Output: a VCF
on standard output (header from mchap_amd.vcfheader, records from mchap_amd.application).

Differences, by design: `--cores N` sizes the pool of host threads that inflate and parse the alignment files (the
reference forks N processes over blocks of loci; here a block of loci is one GPU launch); with several ranks
(`python -m torch.distributed.run --nproc-per-node N -m mchap_amd ...`, one rank per GPU) the targets / records are
sharded over the ranks and rank 0 writes the one VCF; `--reference` may name a FASTA whose file is absent when its
`.fai` index is present (contig lengths for the header; unknown reference bases are written as N); `--block-path
{auto,off,on,wide}` chooses the host path of a block of targets / records (the block_path keyword of the programs); `call-exact
--estimate-prior-frequencies N [--estimate-tolerance EPS]` estimates every record's prior allele frequencies before it is called
(application.estimate_prior_frequencies); `call-exact --model-evidence FILE [--evidence-ploidy K ...] [--evidence-inbreeding F ...]`
also writes a table of every sample's log evidence under candidate (ploidy, inbreeding) pairs (application.ModelEvidence) and leaves
the VCF, header included, as it is without those flags; so does `call-exact --snv-calls FILE [--snv-report GP]`, which writes the
SNV-level VCF `atomize` would make of the run's output with GQ, DS and ACP from the exact SNV genotype posteriors
(application.SnvCalls), and `call-exact --allele-depths FILE`, which writes the run's VCF again with ADP, the posterior expected read
depth of every allele (application.AlleleDepths), and `call-exact --cross-calls FILE --cross-parents P Q`, which writes the run's VCF
again with the progeny of that cross called under their parents' cross prior (application.CrossCalls), and `call-exact --family-calls
FILE --cross-parents P Q`, which writes it with the parents and the progeny called jointly (application.FamilyCalls), and `call-exact
--parentage FILE --parentage-candidates A B ... [--parentage-progeny C ...] [--parentage-gamete-error E] [--parentage-top N]
[--parentage-selfings]`, which writes a table that ranks every pair of candidate parents per progeny -- with --parentage-selfings every
self of a candidate too -- (application.Parentage), and `call-exact --identity FILE
[--identity-samples A B ...] [--identity-error E] [--identity-min-log-bf X]`, which writes a table that ranks the pairs of samples
by the evidence that they are one individual (application.Identity).  `atomize --haplotypes FILE` is host only (mchap_amd/atomize.py)."""
import argparse
import sys

from . import __version__

PROGRAMS = ("assemble", "call", "call-exact", "find-snvs", "atomize")


def _flag(p, name, dest, action, help):
    p.add_argument(name, dest=dest, action=action, default=(action == "store_false"), help=help)


class _CallFlag(argparse._StoreAction):
    """A --call-* flag of find-snvs: stored as usual, and its name noted in `call_flags` (a flag given with its default value
    still counts as given)."""

    def __call__(self, parser, namespace, values, option_string=None):
        super().__call__(parser, namespace, values, option_string)
        namespace.call_flags = getattr(namespace, "call_flags", ()) + (option_string,)


def _sample_args(p, dirmul_nargs):
    p.add_argument("--bam", type=str, nargs="+", default=[],
                   help="BAM / SAM file(s), a text file with one path per line, or a text file of sample<TAB>path lines")
    p.add_argument("--ploidy", type=str, nargs=1, default=["2"], help="ploidy of all samples, or a file of sample<TAB>ploidy lines")
    if dirmul_nargs == 2:
        p.add_argument("--use-dirmul-prior", type=str, nargs=2, default=[None, None],
                       help="inbreeding (a value or a file of sample<TAB>value lines) and the INFO field of prior allele frequencies")
    else:
        p.add_argument("--use-dirmul-prior", type=str, nargs=1, default=[None],
                       help="Dirichlet-multinomial prior over all SNV combinations: inbreeding as a value or a file of sample<TAB>value lines")
    p.add_argument("--sample-pool", type=str, nargs=1, default=[None],
                   help="pool samples into one genotype: the name of a single pool of all samples, or a file of sample<TAB>pool lines")


def _read_args(p):
    p.add_argument("--base-error-rate", type=float, nargs=1, default=[0.0024])
    _flag(p, "--use-base-phred-scores", "ignore_base_phred_scores", "store_false", "use the base phred scores as a source of error")
    p.add_argument("--mapping-quality", type=int, nargs=1, default=[20], help="minimum mapping quality of the reads used")
    _flag(p, "--keep-duplicate-reads", "skip_duplicates", "store_false", "use reads marked as duplicates")
    _flag(p, "--keep-qcfail-reads", "skip_qcfail", "store_false", "use reads marked as qcfail")
    _flag(p, "--keep-supplementary-reads", "skip_supplementary", "store_false", "use reads marked as supplementary")
    p.add_argument("--read-group-field", type=str, nargs=1, default=["SM"], help='read-group field used as the sample id: "SM" or "ID"')


def _mcmc_args(p):
    p.add_argument("--mcmc-chains", type=int, nargs=1, default=[2])
    p.add_argument("--mcmc-steps", type=int, nargs=1, default=[2000])
    p.add_argument("--mcmc-burn", type=int, nargs=1, default=[1000])
    p.add_argument("--mcmc-seed", type=int, nargs=1, default=[42])
    p.add_argument("--mcmc-chain-incongruence-threshold", type=float, nargs=1, default=[0.60])


def build_parser(program):
    """The parser of one program: the flags of the reference's argument table for it (application/arguments.py:742-838)."""
    p = argparse.ArgumentParser("mchap_amd " + program)
    if program == "atomize":
        # (reference application/atomize.py main: its one flag)
        p.add_argument("--haplotypes", type=str, nargs=1, default=[None],
                       help="VCF (text or bgzip) of haplotype calls to split into basis SNVs; it must carry INFO/SNVPOS.  INFO/DP and "
                            "FORMAT/DP come from FORMAT/SNVDP, INFO/ACP and FORMAT/DS from FORMAT/ACP or FORMAT/AFP where present "
                            "(normalised where they do not sum to the ploidy or to one)")
        return p
    if program == "find-snvs":
        # (reference application/find_snvs.py main: its argument list; --cores as the other programs have it)
        p.add_argument("--targets", type=str, nargs=1, default=[None], help="BED file (3+ columns) of the intervals to search")
        p.add_argument("--reference", type=str, nargs=1, default=[None], help="reference FASTA")
        p.add_argument("--bam", type=str, nargs="+", default=[],
                       help="BAM / SAM file(s), a text file with one path per line, or a text file of sample<TAB>path lines")
        p.add_argument("--maf", type=float, nargs=1, default=[0.0], help="minimum mean of the samples' allele frequencies")
        p.add_argument("--mad", type=int, nargs=1, default=[0], help="minimum allele depth summed over the samples")
        p.add_argument("--ind-maf", type=float, nargs=1, default=[0.1], help="minimum allele frequency within a sample")
        p.add_argument("--ind-mad", type=int, nargs=1, default=[3], help="minimum allele depth within a sample")
        p.add_argument("--min-ind", type=int, nargs=1, default=[1], help="samples that must meet --ind-maf and --ind-mad")
        p.add_argument("--read-group-field", type=str, nargs=1, default=["SM"], help='read-group field used as the sample id: "SM" or "ID"')
        p.add_argument("--mapping-quality", type=int, nargs=1, default=[20], help="minimum mapping quality of the reads counted")
        _flag(p, "--keep-duplicate-reads", "skip_duplicates", "store_false", "count reads marked as duplicates")
        _flag(p, "--keep-qcfail-reads", "skip_qcfail", "store_false", "count reads marked as qcfail")
        _flag(p, "--keep-supplementary-reads", "skip_supplementary", "store_false", "count reads marked as supplementary")
        p.add_argument("--cores", type=int, nargs=1, default=[1], help="host threads reading the alignment files")
        # (not reference flags: the reference's find-snvs leaves every GT null)
        p.add_argument("--call-genotypes", type=str, nargs=1, default=[None], metavar="PLOIDY", action=_CallFlag,
                       help="call each sample's genotype from its allele depths (GT:GPM:AD): the ploidy of all samples, or a file of "
                            "sample<TAB>ploidy lines")
        p.add_argument("--call-inbreeding", type=str, nargs=1, default=[None], metavar="F", action=_CallFlag,
                       help="with --call-genotypes: Dirichlet-multinomial prior with this inbreeding (0 <= F < 1), a value or a file "
                            "of sample<TAB>value lines")
        p.add_argument("--call-prior", type=str, nargs=1, default=["FLAT"], choices=["FLAT", "ADMF"], action=_CallFlag,
                       help="with --call-genotypes: prior allele frequencies, FLAT or the record's ADMF; ADMF without --call-inbreeding "
                            "means F = 0")
        p.add_argument("--call-error-rate", type=float, nargs=1, default=[0.0024], action=_CallFlag,
                       help="with --call-genotypes: base error rate")
        return p
    if program == "assemble":
        _sample_args(p, 1)
        p.add_argument("--reference", type=str, nargs=1, default=[None], help="reference FASTA")
        p.add_argument("--reference-index-only", action="store_true",
                       help="(not a reference flag) accept a --reference of which only the .fai index exists: N for unknown bases")
        p.add_argument("--region", type=str, nargs=1, default=[None], help="a single target contig:start-stop (not with --targets)")
        p.add_argument("--region-id", type=str, nargs=1, default=[None])
        p.add_argument("--targets", type=str, nargs=1, default=[None], help="BED4 file of target loci")
        p.add_argument("--variants", type=str, nargs=1, default=[None], help="VCF (text or bgzip) of the SNVs to assemble over")
        _read_args(p)
        _mcmc_args(p)
        p.add_argument("--mcmc-fix-homozygous", type=float, nargs=1, default=[0.999])
        p.add_argument("--mcmc-llk-cache-threshold", type=int, nargs=1, default=[100])
        p.add_argument("--mcmc-recombination-step-probability", type=float, nargs=1, default=[0.5])
        p.add_argument("--mcmc-dosage-step-probability", type=float, nargs=1, default=[1.0])
        p.add_argument("--mcmc-partial-dosage-step-probability", type=float, nargs=1, default=[0.5])
        p.add_argument("--mcmc-temperatures", type=str, nargs="*", default=["1.0"],
                       help="inverse temperatures of parallel tempered chains, or a file of sample<TAB>t1<TAB>t2... lines")
        p.add_argument("--haplotype-posterior-threshold", type=float, nargs=1, default=[0.20])
    else:
        _sample_args(p, 2)
        p.add_argument("--reference", type=str, nargs=1, default=[None], help="reference FASTA (only needed for CRAM input: not read)")
        p.add_argument("--haplotypes", type=str, nargs=1, default=[None], help="VCF (text or bgzip) of known haplotypes")
        p.add_argument("--filter-input-haplotypes", type=str, nargs=1, default=[None],
                       help="'<field><operator><value>': INFO field of Number A or R, one of = > < >= <= !=, a number")
        p.add_argument("--prior-frequencies", type=str, nargs=1, default=[None],
                       help="INFO field of prior allele frequencies (the second value of --use-dirmul-prior)")
        _read_args(p)
        if program == "call":
            _mcmc_args(p)
        else:
            p.add_argument("--estimate-prior-frequencies", type=int, nargs=1, default=[None], metavar="N",
                           help="(not a reference flag) estimate each record's prior allele frequencies before it is called: at most N "
                                "rounds of the samples' posterior allele frequencies (INFO/AFP) fed back as the prior, from "
                                "--prior-frequencies or flat; needs --use-dirmul-prior; the records carry INFO/EMIT")
            p.add_argument("--estimate-tolerance", type=float, nargs=1, default=[None], metavar="EPS",
                           help="(not a reference flag) with --estimate-prior-frequencies: stop a record once no frequency moves by "
                                "EPS or more (default 1e-6)")
            p.add_argument("--model-evidence", type=str, nargs=1, default=[None], metavar="FILE",
                           help="(not a reference flag) write to FILE, when the run ends, a table of the log evidence of every sample's "
                                "reads under candidate (ploidy, inbreeding) pairs, summed over the records that are called")
            p.add_argument("--evidence-ploidy", type=int, nargs="+", default=None, metavar="K",
                           help="(not a reference flag) with --model-evidence: candidate ploidies, 1 to 15, for every sample (default: "
                                "the sample's own)")
            p.add_argument("--evidence-inbreeding", type=float, nargs="+", default=None, metavar="F",
                           help="(not a reference flag) with --model-evidence: candidate inbreeding values, 0 <= F < 1, for every sample "
                                "(default: the sample's own); needs --use-dirmul-prior")
            p.add_argument("--snv-calls", type=str, nargs=1, default=[None], metavar="FILE",
                           help="(not a reference flag) write to FILE, when the run ends, the SNV-level VCF `atomize` would make of this "
                                "run's output (one record per basis SNV, GT:GQ:PQ:DP:DS), with GQ, DS and INFO/ACP from the exact SNV "
                                "genotype posteriors")
            p.add_argument("--allele-depths", type=str, nargs=1, default=[None], metavar="FILE",
                           help="(not a reference flag) write to FILE, when the run ends, this run's VCF with one field added: ADP, the "
                                "posterior expected read depth of every allele (FORMAT per sample, INFO their sum; Number=R, so FILE "
                                "serves as --haplotypes with --filter-input-haplotypes \"ADP>=1\")")
            p.add_argument("--cross-calls", type=str, nargs=1, default=[None], metavar="FILE",
                           help="(not a reference flag) write to FILE, when the run ends, this run's VCF with three FORMAT fields added "
                                "for the progeny of the cross --cross-parents: CGT, the genotype under the prior the parents' posteriors "
                                "imply, CGPM, its probability, and CLBF, the log Bayes factor of that prior against the calling prior")
            p.add_argument("--family-calls", type=str, nargs=1, default=[None], metavar="FILE",
                           help="(not a reference flag) write to FILE, when the run ends, this run's VCF with the family of the cross "
                                "--cross-parents called jointly: FORMAT FGT, the genotype of a parent or a progeny in the exact joint "
                                "posterior of both parents and all progeny, FGPM, its probability, FLBF (progeny), the log Bayes factor "
                                "of the sample's reads given the rest of the family against its calling prior, and INFO FLBF, that of "
                                "the family against unrelated samples")
            p.add_argument("--cross-parents", type=str, nargs=2, default=None, metavar=("P", "Q"),
                           help="(not a reference flag) with --cross-calls or --family-calls: the two parents of the cross, by sample name")
            p.add_argument("--cross-progeny", type=str, nargs="+", default=None, metavar="SAMPLE",
                           help="(not a reference flag) with --cross-calls: the progeny of the cross (default: every other sample whose "
                                "ploidy is half of P's plus half of Q's)")
            p.add_argument("--gamete-error", type=float, nargs="+", default=None, metavar="E",
                           help="(not a reference flag) with --cross-calls: the probability that a gamete is drawn from the population "
                                "and not from its parent, one value or one for P and one for Q, in [0, 1] (default: 0.01)")
            p.add_argument("--parentage", type=str, nargs=1, default=[None], metavar="FILE",
                           help="(not a reference flag) write to FILE, when the run ends, a table that ranks, for every progeny, every "
                                "pair of the candidate parents --parentage-candidates -- and every candidate with an unknown parent -- by "
                                "the log Bayes factor of the cross model of --cross-calls against unrelated, summed over the records")
            p.add_argument("--parentage-candidates", type=str, nargs="+", default=None, metavar="SAMPLE",
                           help="(not a reference flag) with --parentage: the candidate parents, by sample name, each of even ploidy")
            p.add_argument("--parentage-progeny", type=str, nargs="+", default=None, metavar="SAMPLE",
                           help="(not a reference flag) with --parentage: the progeny (default: every sample that is not a candidate)")
            p.add_argument("--parentage-gamete-error", type=float, nargs=1, default=[None], metavar="E",
                           help="(not a reference flag) with --parentage: the probability that a gamete is drawn from the population and "
                                "not from its parent, one value in [0, 1] for every candidate (default: 0.01)")
            p.add_argument("--parentage-top", type=int, nargs=1, default=[None], metavar="N",
                           help="(not a reference flag) with --parentage: keep the first N rows of every progeny (default 0: all)")
            p.add_argument("--parentage-selfings", action="store_true",
                           help="(not a reference flag) with --parentage: also rank, per progeny, the self (i, i) of every candidate of "
                                "the progeny's ploidy -- two meioses of one genotype drawn from the candidate's posterior")
            p.add_argument("--identity", type=str, nargs=1, default=[None], metavar="FILE",
                           help="(not a reference flag) write to FILE, when the run ends, a table that ranks the pairs of samples of one "
                                "ploidy and one calling prior by the log Bayes factor of 'one genotype, read twice' against unrelated, "
                                "summed over the records")
            p.add_argument("--identity-samples", type=str, nargs="+", default=None, metavar="SAMPLE",
                           help="(not a reference flag) with --identity: the samples compared, by name (default: every sample)")
            p.add_argument("--identity-error", type=float, nargs=1, default=[None], metavar="E",
                           help="(not a reference flag) with --identity: the probability that at a record the two genotypes are "
                                "independent even for one individual, one value in [0, 1] (default: 0.01)")
            p.add_argument("--identity-min-log-bf", type=float, nargs=1, default=[None], metavar="X",
                           help="(not a reference flag) with --identity: keep the rows with LOG_BF >= X (default: all rows)")
            p.add_argument("--snv-report", type=str, nargs="+", default=None, metavar="FIELD", choices=["GP"],
                           help="(not a reference flag) with --snv-calls: GP adds the SNV genotype posteriors as a sixth FORMAT field")
    p.add_argument("--report", type=str, nargs="*", default=[],
                   help="extra fields: AFPRIOR ACP AFP AOP AOPSUM GP GL SNVDP, optionally with an INFO/ or FORMAT/ prefix")
    p.add_argument("--cores", type=int, nargs=1, default=[1], help="host threads reading the alignment files")
    p.add_argument("--block-path", type=str, default="auto", choices=sorted(BLOCK_PATHS),
                   help="(not a reference flag) host path of a block of targets / records: auto = the program's default, off = locus "
                        "by locus, on = as array operations over the block (fails for inputs that path does not take), wide = that "
                        "path with --use-base-phred-scores and --sample-pool too")
    return p


# --block-path -> the block_path keyword of application.assemble / call / call_exact
BLOCK_PATHS = {"auto": None, "off": False, "on": True, "wide": "wide"}


def _ranks():
    """(rank, world, dist) when launched under torch.distributed.run with more than one rank, else (0, 1, None)."""
    import os

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1, None
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    if torch.cuda.is_available():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    if not dist.is_initialized():
        # RCCL needs one GPU per rank; MCHAP_DIST_BACKEND=gloo runs several ranks on one GPU (how it is tested)
        dist.init_process_group(backend=os.environ.get("MCHAP_DIST_BACKEND", "nccl" if torch.cuda.device_count() >= world else "gloo"))
    return rank, world, dist


def run(argv, out=None):
    """argv as sys.argv (argv[1] names the program).  Writes the VCF to `out` (default stdout; with several ranks: rank 0
    only); returns the number of records this process formatted."""
    from . import application, io, vcfheader

    out = out or sys.stdout
    program = argv[1]
    parser = build_parser(program)
    args = parser.parse_args(argv[2:])
    header_argv = [argv[1]] + _header_argv(argv[2:], [o for o in parser._option_string_actions if o.startswith("--")])
    if program == "find-snvs":
        return _run_find_snvs(argv, args, out)
    if program == "atomize":
        return _run_atomize(argv, args, out)
    # must have some source of error in reads (application/arguments.py:1190-1195)
    if args.ignore_base_phred_scores and args.base_error_rate[0] == 0.0:
        raise ValueError("Cannot ignore base phred scores if --base-error-rate is 0")
    id_field = args.read_group_field[0]
    if id_field not in ("SM", "ID"):
        raise ValueError('--read-group-field must be "SM" or "ID"')
    sample_bams = io.sample_pools(io.sample_bam_table(args.bam, id_field), args.sample_pool[0])
    samples = list(sample_bams)
    ploidy = io.sample_values(args.ploidy[0], samples, int)
    report = list(args.report)
    vcfheader.report_fields(report)  # (unknown names fail here, before any work)
    rank, world, dist = _ranks()
    shard = (rank, world) if world > 1 else None
    source = application.ReadSource(sample_bams, error_rate=args.base_error_rate[0], use_phred=not args.ignore_base_phred_scores,
                                    read_group_field=id_field, mapping_quality=args.mapping_quality[0],
                                    skip_duplicates=args.skip_duplicates, skip_qcfail=args.skip_qcfail,
                                    skip_supplementary=args.skip_supplementary, workers=args.cores[0])
    seed = evidence = snv_calls = allele_depths = cross_calls = family_calls = parentage = identity = header = None
    block_path = BLOCK_PATHS[args.block_path]
    if program == "assemble":
        if args.targets[0] is not None and args.region[0] is not None:
            raise ValueError("Cannot combine --targets and --region arguments.")
        if args.variants[0] is None or args.reference[0] is None:
            raise ValueError("--variants and --reference are required")
        seed = args.mcmc_seed[0]
        inbreeding = io.sample_values(args.use_dirmul_prior[0], samples, float)
        reference = io.Reference(args.reference[0], allow_index_only=args.reference_index_only)
        contigs = reference.contigs
        targets = application.assemble_targets(args.targets[0], args.region[0], args.region_id[0])
        records = application.assemble(
            None, args.variants[0], reference, source, ploidy=ploidy, inbreeding=inbreeding, steps=args.mcmc_steps[0],
            burn=args.mcmc_burn[0], chains=args.mcmc_chains[0], seed=seed, haplotype_posterior_threshold=args.haplotype_posterior_threshold[0],
            incongruence_threshold=args.mcmc_chain_incongruence_threshold[0], report=report,
            temperatures=io.sample_temperatures(args.mcmc_temperatures, samples), targets=targets, shard=shard,
            fix_homozygous=args.mcmc_fix_homozygous[0], recombination_step_probability=args.mcmc_recombination_step_probability[0],
            partial_dosage_step_probability=args.mcmc_partial_dosage_step_probability[0],
            dosage_step_probability=args.mcmc_dosage_step_probability[0], llk_cache_threshold=args.mcmc_llk_cache_threshold[0],
            block_path=block_path)
    else:
        if args.haplotypes[0] is None:
            raise ValueError("--haplotypes is required")
        inb_arg, tag = args.use_dirmul_prior
        tag = tag or args.prior_frequencies[0]
        inbreeding = io.sample_values(inb_arg, samples, float)
        contigs = io.vcf_contigs(args.haplotypes[0]) or (io.bam_header(next(iter(source.bams)))[0] if source.bams else [])
        if program == "call-exact":
            estimate = args.estimate_prior_frequencies[0]
            if estimate is None and args.estimate_tolerance[0] is not None:
                raise ValueError("--estimate-tolerance needs --estimate-prior-frequencies")
            if estimate is not None and estimate < 0:
                raise ValueError("--estimate-prior-frequencies: N >= 0")
            if estimate is not None and inbreeding is None:
                raise ValueError("--estimate-prior-frequencies needs --use-dirmul-prior: the flat genotype prior has no allele "
                                 "frequencies to estimate")
            evidence = model_evidence_settings(args, samples, inbreeding, tag, estimate, world)
            snv_calls = snv_calls_settings(args, samples, world, ["mchap_amd"] + header_argv)
            if args.allele_depths[0] is not None or args.cross_calls[0] is not None or args.family_calls[0] is not None:
                header = vcfheader.header_lines(program, ["mchap_amd"] + header_argv, samples, contigs, report=report, random_seed=seed,
                                                estimate=estimate is not None)
            allele_depths = allele_depths_settings(args, samples, world, header)
            cross_calls = cross_calls_settings(args, samples, ploidy, world, header)
            family_calls = family_calls_settings(args, samples, ploidy, world, header)
            parentage = parentage_settings(args, samples, ploidy, inbreeding, tag, estimate, world)
            identity = identity_settings(args, samples, ploidy, inbreeding, tag, estimate, world)
            records = application.call_exact(args.haplotypes[0], source, ploidy=ploidy, report=report, prior_frequencies_tag=tag,
                                             inbreeding=inbreeding, filter_input_haplotypes=args.filter_input_haplotypes[0], shard=shard,
                                             block_path=block_path, estimate_frequencies=estimate,
                                             estimate_tolerance=1e-6 if args.estimate_tolerance[0] is None else args.estimate_tolerance[0],
                                             model_evidence=evidence, snv_calls=snv_calls, allele_depths=allele_depths,
                                             cross_calls=cross_calls, family_calls=family_calls, parentage=parentage,
                                             identity=identity)
        else:
            seed = args.mcmc_seed[0]
            records = application.call(args.haplotypes[0], source, ploidy=ploidy, report=report, prior_frequencies_tag=tag,
                                       inbreeding=inbreeding, steps=args.mcmc_steps[0], burn=args.mcmc_burn[0], chains=args.mcmc_chains[0],
                                       seed=seed, incongruence_threshold=args.mcmc_chain_incongruence_threshold[0],
                                       filter_input_haplotypes=args.filter_input_haplotypes[0], shard=shard, block_path=block_path)
    lines = list(records) if world > 1 else records
    if world > 1:
        # the only exchange: every rank's formatted record lines to rank 0, which writes them in target order (the shards
        # are contiguous, so rank order is target order)
        gathered = [None] * world if rank == 0 else None
        dist.gather_object(lines, gathered, dst=0)
        n_mine = len(lines)
        if rank != 0:
            return n_mine
        lines = [ln for part in gathered for ln in part]
    if header is None:   # (--allele-depths and --cross-calls have formed it already: their files carry the very same lines)
        header = vcfheader.header_lines(program, ["mchap_amd"] + header_argv, samples, contigs, report=report, random_seed=seed,
                                        estimate=program == "call-exact" and args.estimate_prior_frequencies[0] is not None)
    for line in header:
        out.write(line + "\n")
    n = 0
    run.limit_records = 0
    for line in lines:
        out.write(line + "\n")
        n += 1
        if program == "assemble" and line.split("\t", 7)[6] == "LIMIT":
            run.limit_records += 1  # (a target beyond the build's shape limits: written with null genotypes, and main() says so)
    if program == "call-exact" and evidence is not None:
        evidence.write(args.model_evidence[0])
    if snv_calls is not None:
        snv_calls.write(args.snv_calls[0])
    if allele_depths is not None:
        allele_depths.write(args.allele_depths[0])
    if cross_calls is not None:
        cross_calls.write(args.cross_calls[0])
    if family_calls is not None:
        family_calls.write(args.family_calls[0])
    if parentage is not None:
        parentage.write(args.parentage[0])
    if identity is not None:
        identity.write(args.identity[0])
    return n


EVIDENCE_FLAGS = ("--model-evidence", "--evidence-ploidy", "--evidence-inbreeding")
# the flags of the SNV file: left out of the header's command line as the evidence flags are
SNV_FLAGS = ("--snv-calls", "--snv-report")
# ... and the flag of the allele-depths file
ALLELE_DEPTH_FLAGS = ("--allele-depths",)
# ... and the flags of the cross-calls file
CROSS_FLAGS = ("--cross-calls", "--cross-parents", "--cross-progeny", "--gamete-error")
# ... and the flag of the family-calls file, which takes its cross from the three above
FAMILY_FLAGS = ("--family-calls",)
# ... and the flags of the parentage table
PARENTAGE_FLAGS = ("--parentage", "--parentage-candidates", "--parentage-progeny", "--parentage-gamete-error", "--parentage-top")
# ... and the flag of its selfing rows, in a tuple of its own
PARENTAGE_SELFING_FLAGS = ("--parentage-selfings",)
# ... and the flags of the identity table
IDENTITY_FLAGS = ("--identity", "--identity-samples", "--identity-error", "--identity-min-log-bf")


def _header_argv(argv, options):
    """The command line as the VCF header states it: without the model-evidence, SNV-file, allele-depths, cross-calls, family-calls, parentage and identity flags and their values -- the VCF, header included,
    is byte for byte what the run writes without them.  options: the parser's option strings; a flag is resolved as argparse
    resolves it (the exact name, else the one option it is a prefix of), so an abbreviated flag is taken out too."""
    out, skipping = [], False
    for a in argv:
        if a.startswith("--"):
            name = a.split("=", 1)[0]
            full = [name] if name in options else [o for o in options if o.startswith(name)]
            skipping = len(full) == 1 and full[0] in EVIDENCE_FLAGS + SNV_FLAGS + ALLELE_DEPTH_FLAGS + CROSS_FLAGS + FAMILY_FLAGS + PARENTAGE_FLAGS + \
                PARENTAGE_SELFING_FLAGS + IDENTITY_FLAGS
        if not skipping:
            out.append(a)
    return out


def model_evidence_settings(args, samples, inbreeding, tag, estimate, world):
    """The --model-evidence / --evidence-* flags of call-exact -> an application.ModelEvidence, or None without --model-evidence
    (any --evidence-* flag is then an error)."""
    from . import application

    if args.model_evidence[0] is None:
        for flag, value in (("--evidence-ploidy", args.evidence_ploidy), ("--evidence-inbreeding", args.evidence_inbreeding)):
            if value is not None:
                raise ValueError("%s needs --model-evidence" % flag)
        return None
    if world > 1:
        raise ValueError("--model-evidence runs as a single process: it does not combine the sums of several ranks (WORLD_SIZE > 1)")
    if args.evidence_ploidy is not None and not all(1 <= K <= 15 for K in args.evidence_ploidy):
        raise ValueError("--evidence-ploidy: candidate ploidies lie in 1..15")
    if args.evidence_inbreeding is not None:
        if inbreeding is None:
            raise ValueError("--evidence-inbreeding needs --use-dirmul-prior: the flat genotype prior has no inbreeding")
        if not all(0.0 <= F < 1.0 for F in args.evidence_inbreeding):   # (False for NaN too)
            raise ValueError("--evidence-inbreeding: candidate values lie in [0, 1)")
    source = "estimated" if estimate is not None else ("flat" if (tag is None or inbreeding is None) else "tag %s" % tag)
    return application.ModelEvidence(samples, args.evidence_ploidy, args.evidence_inbreeding, frequency_source=source)


def snv_calls_settings(args, samples, world, command):
    """The --snv-calls / --snv-report flags of call-exact -> an application.SnvCalls, or None without --snv-calls (--snv-report is
    then an error)."""
    from . import application, atomize

    if args.snv_calls[0] is None:
        if args.snv_report is not None:
            raise ValueError("--snv-report needs --snv-calls")
        return None
    if world > 1:
        raise ValueError("--snv-calls runs as a single process: the SNV file is not gathered from several ranks (WORLD_SIZE > 1)")
    return application.SnvCalls(samples, atomize.vcf_contig_lines(args.haplotypes[0]), report=args.snv_report or (), command=command)


def allele_depths_settings(args, samples, world, header_lines):
    """The --allele-depths flag of call-exact -> an application.AlleleDepths over the run's header lines, or None without it."""
    from . import application

    if args.allele_depths[0] is None:
        return None
    if world > 1:
        raise ValueError("--allele-depths runs as a single process: the file is not gathered from several ranks (WORLD_SIZE > 1)")
    return application.AlleleDepths(samples, header_lines)


def cross_calls_settings(args, samples, ploidy, world, header_lines):
    """The --cross-calls / --cross-parents / --cross-progeny / --gamete-error flags of call-exact -> an application.CrossCalls over
    the run's header lines, or None without --cross-calls (any of the other three is then an error).  The cross is checked here,
    before any work: the sample names, two different parents of even ploidy, progeny of ploidy t_P + t_Q."""
    from . import application

    if args.cross_calls[0] is None:
        if getattr(args, "family_calls", [None])[0] is not None:   # (the cross is --family-calls' then)
            return None
        for flag, value in (("--cross-parents", args.cross_parents), ("--cross-progeny", args.cross_progeny),
                            ("--gamete-error", args.gamete_error)):
            if value is not None:
                raise ValueError("%s needs --cross-calls" % flag)
        return None
    if args.cross_parents is None:
        raise ValueError("--cross-calls needs --cross-parents P Q")
    if world > 1:
        raise ValueError("--cross-calls runs as a single process: the file is not gathered from several ranks (WORLD_SIZE > 1)")
    error = [0.01] if args.gamete_error is None else list(args.gamete_error)
    if len(error) > 2 or not all(0.0 <= e <= 1.0 for e in error):   # (False for NaN too)
        raise ValueError("--gamete-error: one value, or one for each parent, in [0, 1]")
    calls = application.CrossCalls(samples, args.cross_parents, args.cross_progeny, error, header_lines)
    calls.cross.resolve(list(samples), application._per_sample(ploidy, samples))
    return calls


def family_calls_settings(args, samples, ploidy, world, header_lines):
    """The --family-calls flag of call-exact, with the cross of --cross-parents / --cross-progeny / --gamete-error -> an
    application.FamilyCalls over the run's header lines, or None without --family-calls.  The cross is checked here, before any
    work, as cross_calls_settings checks it."""
    from . import application

    if args.family_calls[0] is None:
        return None
    if args.cross_parents is None:
        raise ValueError("--family-calls needs --cross-parents P Q")
    if world > 1:
        raise ValueError("--family-calls runs as a single process: the file is not gathered from several ranks (WORLD_SIZE > 1)")
    error = [0.01] if args.gamete_error is None else list(args.gamete_error)
    if len(error) > 2 or not all(0.0 <= e <= 1.0 for e in error):   # (False for NaN too)
        raise ValueError("--gamete-error: one value, or one for each parent, in [0, 1]")
    calls = application.FamilyCalls(samples, args.cross_parents, args.cross_progeny, error, header_lines)
    calls.cross.resolve(list(samples), application._per_sample(ploidy, samples))
    return calls


def identity_settings(args, samples, ploidy, inbreeding, tag, estimate, world):
    """The --identity / --identity-* flags of call-exact -> an application.Identity, or None without --identity (any --identity-*
    flag is then an error).  The pairs are checked here, before any work: the sample names, none twice, at least two, the error in
    [0, 1]."""
    from . import application

    if args.identity[0] is None:
        for flag, value in (("--identity-samples", args.identity_samples), ("--identity-error", args.identity_error[0]),
                            ("--identity-min-log-bf", args.identity_min_log_bf[0])):
            if value is not None:
                raise ValueError("%s needs --identity" % flag)
        return None
    if world > 1:
        raise ValueError("--identity runs as a single process: it does not combine the sums of several ranks (WORLD_SIZE > 1)")
    error = 0.01 if args.identity_error[0] is None else args.identity_error[0]
    if not 0.0 <= error <= 1.0:   # (False for NaN too)
        raise ValueError("--identity-error: one value in [0, 1]")
    least = args.identity_min_log_bf[0]
    if least is not None and least != least:
        raise ValueError("--identity-min-log-bf: a number")
    source = "estimated" if estimate is not None else ("flat" if (tag is None or inbreeding is None) else "tag %s" % tag)
    table = application.Identity(samples, args.identity_samples, error, least, frequency_source=source)
    table.resolve(application._per_sample(ploidy, samples), application._per_sample(inbreeding, samples))
    return table


def parentage_settings(args, samples, ploidy, inbreeding, tag, estimate, world):
    """The --parentage / --parentage-* flags of call-exact -> an application.Parentage, or None without --parentage (any
    --parentage-* flag is then an error).  The hypotheses are checked here, before any work: the sample names, none twice, every
    candidate of even ploidy, the gamete error in [0, 1], N >= 0.  --parentage-selfings (read with getattr: a namespace built by hand
    may lack it) adds the selfing rows."""
    from . import application

    selfings = bool(getattr(args, "parentage_selfings", False))
    if args.parentage[0] is None:
        for flag, value in (("--parentage-candidates", args.parentage_candidates), ("--parentage-progeny", args.parentage_progeny),
                            ("--parentage-gamete-error", args.parentage_gamete_error[0]), ("--parentage-top", args.parentage_top[0]),
                            ("--parentage-selfings", True if selfings else None)):
            if value is not None:
                raise ValueError("%s needs --parentage" % flag)
        return None
    if args.parentage_candidates is None:
        raise ValueError("--parentage needs --parentage-candidates SAMPLE [SAMPLE ...]")
    if world > 1:
        raise ValueError("--parentage runs as a single process: it does not combine the sums of several ranks (WORLD_SIZE > 1)")
    error = 0.01 if args.parentage_gamete_error[0] is None else args.parentage_gamete_error[0]
    if not 0.0 <= error <= 1.0:   # (False for NaN too)
        raise ValueError("--parentage-gamete-error: one value in [0, 1]")
    top = 0 if args.parentage_top[0] is None else args.parentage_top[0]
    if top < 0:
        raise ValueError("--parentage-top: N >= 0")
    source = "estimated" if estimate is not None else ("flat" if (tag is None or inbreeding is None) else "tag %s" % tag)
    table = application.Parentage(samples, args.parentage_candidates, args.parentage_progeny, error, top, frequency_source=source,
                                  selfings=selfings)
    table.resolve(application._per_sample(ploidy, samples))
    return table


def _run_atomize(argv, args, out):
    """atomize: the SNV file of a haplotype VCF on `out`; host only."""
    from . import atomize

    if args.haplotypes[0] is None:
        raise ValueError("--haplotypes is required")
    sys.stderr.write("mchap_amd atomize: the reference marks this program as experimental\n")
    return atomize.atomize_vcf(args.haplotypes[0], out, command=["mchap_amd"] + list(argv[1:]))


def find_snvs_call_settings(args, samples):
    """The --call-* flags of find-snvs -> the `genotypes` settings of find_snvs.find_snvs, or None without --call-genotypes (any
    other --call-* flag is then an error).  There is no prior unless --call-inbreeding or --call-prior ADMF is given."""
    from . import io

    if args.call_genotypes[0] is None:
        for flag in getattr(args, "call_flags", ()):
            raise ValueError("%s needs --call-genotypes" % flag)
        return None
    ploidy = io.sample_values(args.call_genotypes[0], samples, int)
    inbreeding = io.sample_values(args.call_inbreeding[0], samples, float)
    for name, values, ok in (("--call-genotypes", ploidy, lambda v: v >= 1), ("--call-inbreeding", inbreeding, lambda v: 0.0 <= v < 1.0)):
        for v in (values.values() if isinstance(values, dict) else [] if values is None else [values]):
            if not ok(v):
                raise ValueError("%s: %r is out of range" % (name, v))
    error_rate = args.call_error_rate[0]
    if not 0.0 <= error_rate < 1.0:
        raise ValueError("--call-error-rate must be in [0, 1)")
    return dict(ploidy=ploidy, inbreeding=inbreeding, frequencies="ADMF" if args.call_prior[0] == "ADMF" else None, error_rate=error_rate)


def _run_find_snvs(argv, args, out):
    """find-snvs: the header, then the records of every BED interval in file order (one process: sharding is out of scope)."""
    import os

    from . import application, find_snvs, io, vcfheader

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("find-snvs runs as a single process: it does not shard over several ranks (WORLD_SIZE > 1)")
    if args.targets[0] is None or args.reference[0] is None:
        raise ValueError("--targets and --reference are required")
    id_field = args.read_group_field[0]
    if id_field not in ("SM", "ID"):
        raise ValueError('--read-group-field must be "SM" or "ID"')
    sample_bams = io.sample_bam_table(args.bam, id_field)
    find_snvs.check_one_sample_per_file(sample_bams, id_field)
    reference = io.Reference(args.reference[0])
    targets = find_snvs.read_targets(args.targets[0])
    source = application.ReadSource(sample_bams, read_group_field=id_field, mapping_quality=args.mapping_quality[0],
                                    skip_duplicates=args.skip_duplicates, skip_qcfail=args.skip_qcfail,
                                    skip_supplementary=args.skip_supplementary, workers=args.cores[0])
    genotypes = find_snvs_call_settings(args, list(sample_bams))
    records = find_snvs.find_snvs(targets, reference, source, maf=args.maf[0], mad=args.mad[0], ind_maf=args.ind_maf[0],
                                  ind_mad=args.ind_mad[0], min_ind=args.min_ind[0], genotypes=genotypes)
    lines = list(records)  # (errors -- an interval past its contig's end -- surface before any output)
    for line in vcfheader.find_snvs_header_lines(["mchap_amd"] + list(argv[1:]), args.reference[0], list(sample_bams), reference.contigs,
                                                 genotypes=genotypes is not None):
        out.write(line + "\n")
    for line in lines:
        out.write(line + "\n")
    return len(lines)


def main(argv=None):
    argv = sys.argv if argv is None else argv
    parser = argparse.ArgumentParser("MI355X-native MCHap programs")
    parser.add_argument("-v", "--version", action="version", version="mchap_amd %s" % __version__)
    parser.add_argument("program", nargs=1, choices=PROGRAMS, help="sub-program")
    if len(argv) < 2:
        parser.print_help()
        return 0
    parser.parse_args(argv[1:2])
    run(argv)
    if getattr(run, "limit_records", 0):
        sys.stderr.write("mchap_amd: %d target(s) were not assembled (FILTER=LIMIT): exit status 3\n" % run.limit_records)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())
