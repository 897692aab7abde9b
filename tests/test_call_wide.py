"""CPU: `mchap call` over more than 256 known haplotypes -- the library's bound and workspace figures (no device needed: they are
plain functions of the shape), and the program `application.call` with the sampler stubbed: a record of 300 alternate alleles is
called like its neighbours and leaves their lines alone, a record beyond mchap_call_mcmc_max_haps is a FILTER=LIMIT record.

And the checker itself beyond 256 haplotypes: the oracle's sampler against the reference's own (tests/golden/call_wide_traces.npz,
made by tests/golden/make_call_wide.py), its genotype counts and ranks against exact integers up to the 2^62 bound."""
import io as _io
import math
import os

import numpy as np
import pytest

from tests.call_wide_helpers import largest_haps_below_2_62, rank_cases, wide_vcf

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")
DEEP = ["simple.sample1.deep.bam", "simple.sample2.deep.bam", "simple.sample3.deep.bam"]


def test_bound_and_workspace_figures(monkeypatch):
    from mchap_amd import _lib

    monkeypatch.delenv("MCHAP_HIP_CALL_WIDE", raising=False)
    L = _lib.lib()
    assert "mchap_call_mcmc_max_haps" in _lib.EXPORTS
    for K in range(2, 9):
        assert int(L.mchap_call_mcmc_max_haps(K)) >= 1024
    assert int(L.mchap_call_mcmc_max_haps(0)) == 0 and int(L.mchap_call_mcmc_max_haps(99)) == 0
    K, R, S, Cn = 4, 100, 2000, 2
    for H in (300, 1024):
        base = int(L.mchap_call_mcmc_workspace_bytes(1, H, K, S, Cn))
        one = int(L.mchap_call_mcmc_workspace_bytes_for(1, R, H, K, S, Cn))
        # the likelihood tables (2 x steps x K x H entries of 16 bytes a chain, a power of two) and the unit's product table, once
        assert base >= Cn * 2 * S * K * H * 16
        assert R * H * 8 <= one - base < 2 * R * H * 8 + (3 * K + 4) * H * 8 + 4096
        # ... linear in the units: application.call sizes its sub-batches with the figure of one unit
        assert int(L.mchap_call_mcmc_workspace_bytes_for(7, R, H, K, S, Cn)) == 7 * one
    # up to 256 haplotypes the figure is what it was, and MCHAP_HIP_CALL_WIDE=1 sizes the other path's
    narrow = int(L.mchap_call_mcmc_workspace_bytes_for(3, R, 16, K, S, Cn))
    monkeypatch.setenv("MCHAP_HIP_CALL_WIDE", "1")
    forced = int(L.mchap_call_mcmc_workspace_bytes_for(3, R, 16, K, S, Cn))
    base = int(L.mchap_call_mcmc_workspace_bytes(3, 16, K, S, Cn))
    assert narrow > base and forced >= base + 3 * R * 16 * 8 and forced != narrow


def test_call_program_with_a_stubbed_sampler(tmp_path, monkeypatch, capsys):
    from mchap_amd import _lib, application, cli
    from mchap_amd.calling_mcmc import CallingMCMC, CallSummary

    seen = []

    def stub(self, reads, read_counts=None, initial=None, haplotypes=None, prior=None, stream_ids=None, burn=0, incongruence_threshold=0.6,
             max_states=512, stream=None):
        """a unit's genotype from its own reads alone: K copies of the haplotype that matches the reads' mean best"""
        U, H, K = len(reads), haplotypes.shape[1], int(self.ploidy)
        top = int(_lib.lib().mchap_call_mcmc_max_haps(K))
        if H > top:  # (what mchap_call_mcmc_batch_device answers: MCHAP_ERR_LIMIT -> NotImplementedError)
            raise NotImplementedError("mchap_hip: n_haps %d > %d (mchap_call_mcmc_max_haps)" % (H, top))
        seen.append((U, H, K, reads.shape[1], reads.shape[2], reads.shape[3]))
        done = []
        n_obs = int(self.chains) * (int(self.steps) - burn)
        for u in range(U):
            mean = np.nan_to_num(np.nanmean(reads[u], axis=0))                       # [M, A]
            score = mean[np.arange(haplotypes.shape[2])[None, :], haplotypes[u]].sum(axis=1)  # [H]
            a = int(np.argmax(score))
            done.append(CallSummary(genotypes=np.full((1, K), a, np.int32), counts=np.array([n_obs]), n_obs=n_obs, alleles=np.full(K, a, np.int32),
                                    gprob=1.0, sprob=1.0, mci=0, n_allele=H))
        return dict(done=done)

    monkeypatch.setattr(CallingMCMC, "start_batch_summaries", stub)
    monkeypatch.setattr(application, "_call_stream", lambda i: None)
    budgets, budget = [], application.device_unit_budget

    def recording_budget(bytes_per_unit, *a, **kw):
        budgets.append(int(bytes_per_unit))
        return budget(bytes_per_unit, *a, **kw)

    monkeypatch.setattr(application, "device_unit_budget", recording_budget)
    base = os.path.join(HERE, "simple.output.deep.assemble.vcf")
    top = int(_lib.lib().mchap_call_mcmc_max_haps(4))
    with_wide, with_both = str(tmp_path / "wide.vcf"), str(tmp_path / "both.vcf")
    wide_vcf(base, with_wide, [("CHR1", 6, "WIDE300", 300)])
    wide_vcf(base, with_both, [("CHR1", 6, "WIDE300", 300), ("CHR2", 11, "BEYOND", top + 1)])

    def run(vcf):  # (application.call behind the command-line shell)
        out = _io.StringIO()
        cli.run(["mchap_amd", "call", "--bam"] + [os.path.join(HERE, f) for f in DEEP] + ["--ploidy", "4", "--haplotypes", vcf,
                 "--mcmc-steps", "300", "--mcmc-burn", "100", "--mcmc-seed", "5", "--report", "AFP"], out)
        return [ln for ln in out.getvalue().splitlines() if ln and not ln.startswith("#")]

    plain, wide = run(base), run(with_wide)
    capsys.readouterr()
    assert len(wide) == len(plain) + 1
    # the program sized the wide record's sub-batches with the figure that counts the unit's tables (_for), not the smaller one
    (w_shape,) = {t for t in seen if t[1] == 301}
    _, H, K, R, M, A = w_shape
    L = _lib.lib()
    ws1 = int(L.mchap_call_mcmc_workspace_bytes_for(1, R, H, K, 300, 2))
    assert ws1 >= int(L.mchap_call_mcmc_workspace_bytes(1, H, K, 300, 2)) + R * H * 8
    assert R * M * A * 8 + R * 8 + 2 * 300 * (K + 1) * 8 + ws1 + 4096 in budgets
    rec = [ln.split("\t") for ln in wide]
    assert all(f[6] != "LIMIT" for f in rec)
    (w,) = [f for f in rec if f[2] == "WIDE300"]
    assert len(w[4].split(",")) == 300 and all("." not in s.split(":")[0] for s in w[9:])
    assert [ln for ln in wide if ln.split("\t")[2] != "WIDE300"] == plain
    both = run(with_both)
    err = capsys.readouterr().err
    by = {ln.split("\t")[2]: ln.split("\t") for ln in both}
    assert by["BEYOND"][6] == "LIMIT" and by["BEYOND"][9].split(":")[0] == "./././."
    assert "not called" in err and "FILTER=LIMIT" in err and str(top) in err
    assert [ln for ln in both if ln.split("\t")[2] != "BEYOND"] == wide


def test_call_writes_the_samplers_mci_into_its_records(tmp_path, monkeypatch):
    """MCI of `mchap call` is a sampler statistic: per sample in FORMAT field 10, the number of samples above 0 in INFO between NS and DP.
    Two samples of different ploidy (so the stub knows whose units it has), three records, one of them REFMASKED; the stub answers
    mci = 1 for the tetraploid sample's units and 0 for the diploid's, and every other field equals a run where it answers 0 throughout."""
    from mchap_amd import application
    from mchap_amd.calling_mcmc import CallingMCMC, CallSummary

    mci_of = {}

    def stub(self, reads, read_counts=None, initial=None, haplotypes=None, prior=None, stream_ids=None, burn=0, incongruence_threshold=0.6,
             max_states=512, stream=None):
        U, H, K = len(reads), haplotypes.shape[1], int(self.ploidy)
        n_obs = int(self.chains) * (int(self.steps) - burn)
        return dict(done=[CallSummary(genotypes=np.full((1, K), H - 1, np.int32), counts=np.array([n_obs]), n_obs=n_obs,
                                      alleles=np.full(K, H - 1, np.int32), gprob=1.0, sprob=1.0, mci=mci_of[K], n_allele=H) for _ in range(U)])

    monkeypatch.setattr(CallingMCMC, "start_batch_summaries", stub)
    monkeypatch.setattr(application, "_call_stream", lambda i: None)
    vcf = str(tmp_path / "haps.vcf")
    with open(os.path.join(HERE, "simple.output.deep.assemble.vcf")) as fh:
        lines = [ln.rstrip("\n") for ln in fh]
    head = [ln for ln in lines if ln.startswith("#")]
    recs = [ln.split("\t") for ln in lines if not ln.startswith("#") and ln.split("\t")[4] != "."]   # (the two records with SNVs)
    masked = list(recs[1])
    masked[1], masked[2], masked[7] = str(int(masked[1]) + 1), "MASKED", masked[7].replace(";NS=", ";REFMASKED;NS=")
    with open(vcf, "w") as fh:
        fh.write("\n".join(head + ["\t".join(f) for f in recs + [masked]]) + "\n")
    bams = {"SAMPLE1": os.path.join(HERE, DEEP[0]), "SAMPLE2": os.path.join(HERE, DEEP[1])}

    def run():
        return [ln.split("\t") for ln in application.call(vcf, dict(bams), ploidy={"SAMPLE1": 4, "SAMPLE2": 2}, steps=300, burn=100, seed=5)]

    mci_of.update({4: 1, 2: 0})
    got = run()
    mci_of.update({4: 0, 2: 0})
    quiet = run()
    assert len(got) == len(quiet) == 3 and "REFMASKED" in got[2][7].split(";") and all(f[6] == "PASS" for f in got)
    for f, q in zip(got, quiet):
        s1, s2 = f[9].split(":"), f[10].split(":")
        assert len(s1) == len(s2) == 11 and s1[10] == "1" and s2[10] == "0"
        info = f[7].split(";")
        at = info.index("MCI=1")
        assert info[at - 1].startswith("NS=") and info[at + 1].startswith("DP=")
        # everything else as without incongruence
        assert q[9].split(":")[10] == q[10].split(":")[10] == "0" and "MCI=0" in q[7].split(";")
        assert s1[:10] == q[9].split(":")[:10] and s2[:10] == q[10].split(":")[:10]
        assert [x for x in info if x != "MCI=1"] == [x for x in q[7].split(";") if x != "MCI=0"]
        assert f[:7] + f[8:9] == q[:7] + q[8:9]


# ---- the oracle beyond 256 known haplotypes, against the reference ----
def _wide_case(z, i):
    p = "c%d_" % i
    K, F, has_f = z[p + "meta"]
    prior = None if F < 0 else (float(F), z[p + "freqs"] if has_f else None)
    counts = z[p + "counts"]
    return p, int(K), prior, (None if counts.size == 0 else counts)


def test_oracle_beyond_256_transition_vectors_and_greedy_caller(golden_dir):
    """test_oracle_call_mcmc.py::test_transition_vectors_and_greedy_caller (its tolerances) over 300, 321 and 1024 haplotypes, at
    states whose alleles lie above 255."""
    from oracle import binding as orc

    z = np.load(os.path.join(golden_dir, "call_wide_traces.npz"))
    kinds = set()
    for i in range(int(z["n_cases"])):
        p, K, prior, counts = _wide_case(z, i)
        haps, reads = z[p + "haps"], z[p + "reads"]
        kinds.add((None if prior is None else prior[1] is not None, counts is not None))
        assert len(haps) > 256 and (z[p + "states"][:, :K] > 255).any(axis=1).all()
        for state, vec in zip(z[p + "states"], z[p + "vectors"]):
            g, k = state[:K], int(state[K])
            for st in (0, 1):
                llks, lpri, probs = orc.call_step_options(reads, haps, g, k, st, counts, prior)
                np.testing.assert_allclose(llks, vec[st][0], rtol=1e-12)
                np.testing.assert_allclose(lpri, vec[st][1], rtol=1e-12, atol=1e-12, equal_nan=True)
                np.testing.assert_allclose(probs, vec[st][2], rtol=1e-10, atol=1e-300, equal_nan=True)
        assert orc.greedy_caller(reads, haps, K, counts, prior).tolist() == z[p + "greedy"].tolist()
    # no prior, (F, None) and (F, freqs); with and without read counts
    assert {k[0] for k in kinds} == {None, False, True} and {k[1] for k in kinds} == {False, True}


def test_oracle_beyond_256_seeded_fits_step_for_step(golden_dir):
    """test_oracle_call_mcmc.py::test_seeded_fits_step_for_step over the same cases: the reference's CallingMCMC.fit under numpy's
    MT19937, both step types and a fit from a given initial genotype -- alleles equal, llks to 1e-10.  The fixture's traces visit
    alleles above 255 and change genotype, each step type's (or they would pin nothing that 256 haplotypes do not)."""
    from oracle import binding as orc

    z = np.load(os.path.join(golden_dir, "call_wide_traces.npz"))
    n = int(z["n_cases"])
    steps, chains, ini_steps, mh_steps = (int(v) for v in z["steps"])
    shapes = set()
    for i in range(n):
        p, K, prior, counts = _wide_case(z, i)
        haps, reads = z[p + "haps"], z[p + "reads"]
        shapes.add((K, len(haps)))
        beyond = 0
        for st in (0, 1):
            n_steps = mh_steps if st else steps  # (Metropolis-Hastings accepts few proposals: the fixture runs it longer)
            ref_g, ref_l = z[p + "trace%d_g" % st], z[p + "trace%d_l" % st]
            assert ref_g.shape == (chains, n_steps, K), (i, st)
            assert (ref_g[:, 1:] != ref_g[:, :-1]).any(), (i, st)  # each step type's trace changes genotype
            beyond += int((ref_g > 255).sum())
            g, l = orc.call_mcmc(reads, haps, K, steps=n_steps, chains=chains, step_type=st, read_counts=counts, prior=prior,
                                 rng_kind=orc.RNG_NUMPY_MT, seed=100 + i)
            assert np.array_equal(g, ref_g), (i, st)
            np.testing.assert_allclose(l, ref_l, rtol=1e-10)
        # (per case, not per step type: a Metropolis-Hastings chain of a diploid may sit below 256 throughout, while every one of its
        # sub-steps still prices all the options above 255)
        assert beyond > 0, i
        g, l = orc.call_mcmc(reads, haps, K, steps=ini_steps, chains=1, step_type=0, read_counts=counts, prior=prior,
                             initial=z[p + "initial"], rng_kind=orc.RNG_NUMPY_MT, seed=7 + i)
        assert (z[p + "initial"] > 255).any()  # (the start: the first sub-steps price options against an allele beyond 255)
        assert np.array_equal(g, z[p + "trace_ini_g"]), i
        np.testing.assert_allclose(l, z[p + "trace_ini_l"], rtol=1e-10)
    assert {(4, 300), (3, 321), (2, 1024)} <= shapes


def test_oracle_genotype_counts_and_ranks_up_to_the_bound():
    """orc_comb_with_replacement and orc_genotype_alleles_as_index against math.comb for every ploidy 2 to 15 at the largest number
    of haplotypes the 2^62 rule admits, and at the shapes the GPU tests of the wide path use."""
    from oracle import binding as orc

    shapes = [(largest_haps_below_2_62(K), K) for K in range(2, 16)] + [(806, 8), (1024, 7), (4096, 5), (300, 10), (105, 15), (4096, 2)]
    assert (806, 8) in shapes[:14] and (105, 15) in shapes[:14]
    for H, K in shapes:
        G = math.comb(H + K - 1, K)
        assert G < 1 << 62
        assert orc.comb_with_replacement(H, K) == G, (H, K)
        for k in range(1, K + 1):
            assert orc.comb_with_replacement(H, k) == math.comb(H + k - 1, k), (H, k)
        g, exact = rank_cases(K, H)
        assert exact[0] == G - 1 and exact[1] == 0
        for row, e in zip(g, exact):
            assert orc.genotype_alleles_as_index(row) == e, (H, K, row.tolist())
