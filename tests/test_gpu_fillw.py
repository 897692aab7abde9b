"""GPU parity of denovo_fillw_kernel (round 4: the phased sampler's table completion as its own launch -- one workgroup per
chain, one wavefront per distinct request, 128 VGPRs) against the completion inside the exporting launch it replaced (the code of
a visit: structural.py:433-673 through denovo_spec_kernel's spec_structural; tuning flag 1024 selects it).

The tables hold the total move probability of every interval step of a settled chain's genotype; the coasting kernel compares
uniforms with them, so a difference of one unit in the last place would hardly ever show in a trace.  The TABLES are therefore
compared entry for entry, bit for bit (NaN = not evaluated and -1 = no options included) -- and then whole traces of full runs,
hand-back rounds included, with the oracle as the third party on one case."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _first_phase(reads, flags, halve_workspace=False, **kw):
    """First phase of the phased sampler (steps, table completion, first coasting launch) -> the chains' interval tables, read
    back where a fit with that workspace put them (mchap_debug_pipe_memo), and the batch."""
    import torch

    from mchap_amd import DenovoMCMC, _lib
    from mchap_amd.device import DenovoDeviceBatch

    os.environ["MCHAP_HIP_TEST_KERNELS"] = "1"  # mchap_debug_pipe_memo lives in the parity suite's library
    os.environ["MCHAP_HIP_PIPE_STOP"] = "1"
    os.environ["MCHAP_HIP_FLAGS"] = str(flags)
    try:
        model = DenovoMCMC(random_seed=42, kernel=5, **kw)
        b = DenovoDeviceBatch(model, reads)
        assert "phased" in b.sampler_name
        if halve_workspace:
            b.ws_bytes //= 2
        b.run()
        torch.cuda.synchronize()
        U, M = reads.shape[0], reads.shape[2]
        E = M * (M + 1) // 2
        memo = np.zeros((U * model.chains, 2, E), dtype=np.float64)
        f = _lib.lib().mchap_debug_pipe_memo
        f.restype = C.c_int
        rc = f(C.byref(b.cfg), U, _lib.ptr(b.units_host), C.c_void_p(b.d_ws.data_ptr()), _lib.ptr(memo), C.c_int64(b.ws_bytes))
        assert rc == 0, _lib.last_error()
        return memo, b
    finally:
        for k in ("MCHAP_HIP_TEST_KERNELS", "MCHAP_HIP_PIPE_STOP", "MCHAP_HIP_FLAGS"):
            os.environ.pop(k, None)


def _tables(reads, flags, **kw):
    return _first_phase(reads, flags, **kw)[0]


CASES = {
    # name: (units, ploidy, n_pos, n_reads, n_alleles, inbreeding, synth kwargs)
    "config2": (48, 4, 8, 200, 2, None, {}),
    "config2-inbred": (16, 4, 8, 200, 2, 0.1, {}),
    "diploid-20-snvs": (16, 2, 20, 90, 2, None, dict(window=(4, 12))),      # several chunks of entries (420 per table pair)
    "triploid-odd-reads": (16, 3, 7, 131, 2, None, dict(window=(3, 7))),
    "hexaploid": (12, 6, 8, 200, 2, None, {}),                               # 30 + 30 options per interval: several chunks of slots
    "octoploid": (6, 8, 8, 300, 2, None, {}),                                # five read chunks: the block beyond the base products
    "triallelic": (12, 4, 7, 150, 3, None, dict(window=(4, 7))),             # two bits per allele: 56-bit genotypes
    "tetraploid-16-snvs": (8, 4, 16, 200, 2, None, dict(window=(6, 16))),    # the widest packed key: 64 bits
    "shallow": (24, 4, 8, 20, 2, None, dict(qual=(25, 40))),
    # genotypes of more than 64 bits: requests keyed by their changed words, the cache probe verified against the stored words
    "tetraploid-20-snvs-wide": (12, 4, 20, 150, 2, None, dict(window=(6, 20))),
    "triallelic-wide-keys": (12, 4, 12, 150, 3, 0.1, dict(window=(4, 12))),
    "hexaploid-14-snvs-wide": (8, 6, 14, 120, 2, None, dict(window=(5, 14))),
    # ... and deep units on top (more than four read chunks: product rows in the workspace)
    "octoploid-deep-wide": (4, 8, 20, 1000, 2, None, dict(window=(8, 20))),
    "deep-2600-reads": (3, 4, 6, 2600, 2, None, dict(window=(2, 6), qual=(10, 40))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_tables_equal_the_in_kernel_completion(case):
    from mchap_amd.synth import synth_units

    U, K, M, R, A, F, skw = CASES[case]
    reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, n_alleles=A, first_unit=11, **skw)
    kw = dict(ploidy=K, n_alleles=[A] * M, steps=60, chains=2, inbreeding=F)
    new = _tables(reads, 0, **kw)       # the shipped path: denovo_fillw_kernel after the exporting launch
    old = _tables(reads, 1024, **kw)    # tuning flag 1024: the completion inside the exporting launch
    assert new.shape == old.shape
    done = ~np.isnan(old)
    # (entries beyond the unit's non-fixed positions stay NaN; most chains of these batches settle and get complete tables)
    assert done.any(axis=(1, 2)).mean() > 0.5
    assert np.array_equal(np.isnan(new), np.isnan(old))
    assert np.array_equal(new[done].view(np.uint64), old[done].view(np.uint64)), \
        "max |diff| %.3e" % np.nanmax(np.abs(new - old))
    assert (old[done] >= 0).any() and (old[done] == -1.0).any()  # both kinds of entries occur
    # ... and without the probe of the chain's likelihood cache (2048) / without the unit's table in LDS (4096) / without the memo of
    # evaluated requests across a chain's chunks (32768): the same tables
    for flags in (2048, 4096, 2048 | 4096, 32768, 32768 | 2048):
        alt = _tables(reads, flags, **kw)
        assert np.array_equal(np.isnan(alt), np.isnan(old)) and np.array_equal(alt[done].view(np.uint64), old[done].view(np.uint64)), flags


def test_the_reader_follows_the_fit_into_a_smaller_workspace():
    """A fit handed half the bytes mchap_denovo_workspace_bytes asked for halves its likelihood caches and takes the decision
    contexts the rest holds: the pieces behind the caches -- the interval tables among them -- move.  The reader resolves the layout
    as the fit did, so it finds the same tables (and the traces do not depend on either size)."""
    from mchap_amd.synth import synth_units

    reads, _, _ = synth_units(16, ploidy=4, n_pos=8, n_reads=200, first_unit=11)
    kw = dict(ploidy=4, n_alleles=[2] * 8, steps=60, chains=2)
    memo, whole = _first_phase(reads, 0, **kw)
    memo_half, half = _first_phase(reads, 0, halve_workspace=True, **kw)
    assert half.ws_bytes == whole.ws_bytes // 2
    assert (~np.isnan(memo)).any(axis=(1, 2)).mean() > 0.5
    assert np.array_equal(memo, memo_half, equal_nan=True)
    for x, y in zip(whole.traces(), half.traces()):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def _run(reads, flags, **kw):
    import torch

    from mchap_amd import DenovoMCMC
    from mchap_amd.device import DenovoDeviceBatch

    os.environ["MCHAP_HIP_FLAGS"] = str(flags)
    try:
        b = DenovoDeviceBatch(DenovoMCMC(random_seed=7, kernel=5, **kw), reads)
        b.run()
        torch.cuda.synchronize()
        return b.traces()
    finally:
        os.environ.pop("MCHAP_HIP_FLAGS", None)


@pytest.mark.parametrize("case", ["config2", "shallow", "triallelic", "hexaploid"])
def test_whole_traces_do_not_depend_on_the_completion_kernel(case):
    """Full runs (hand-back rounds included: their lists go through the same kernel): words, fixed alleles, llks and status."""
    from mchap_amd.synth import synth_units

    U, K, M, R, A, F, skw = CASES[case]
    reads, _, _ = synth_units(U, ploidy=K, n_pos=M, n_reads=R, n_alleles=A, first_unit=3, **skw)
    kw = dict(ploidy=K, n_alleles=[A] * M, steps=400, chains=2, inbreeding=F)
    a, b = _run(reads, 0, **kw), _run(reads, 1024, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def test_against_the_oracle_step_for_step():
    from oracle import binding as orc

    from mchap_amd.assemble import break_table
    from mchap_amd.classes import sort_haplotypes
    from mchap_amd.device import DenovoDeviceBatch
    from mchap_amd import DenovoMCMC
    from mchap_amd.synth import synth_units
    import torch

    reads, _, _ = synth_units(6, ploidy=4, n_pos=8, n_reads=200, first_unit=500)
    model = DenovoMCMC(ploidy=4, n_alleles=[2] * 8, steps=300, chains=2, random_seed=11, kernel=5)
    b = DenovoDeviceBatch(model, reads)
    assert "phased" in b.sampler_name
    b.run()
    torch.cuda.synchronize()
    words, fixed, llks, status = b.traces()
    assert (status == 0).all()
    for u in range(len(reads)):
        cfg = orc.make_cfg(4, 300, 2, None, (1.0,), llk_cache_threshold=-1, rng_kind=orc.RNG_PHILOX, seed=11, stream_id=u,
                           break_table=break_table(8, 1.0, 3.0))
        g, l, code = orc.denovo_fit(cfg, reads[u], [2] * 8)
        assert code == 0
        assert np.array_equal(b.genotypes(u, words, fixed), sort_haplotypes(g))
        np.testing.assert_allclose(llks[u], l, rtol=1e-10)


def test_a_workspace_reused_for_other_data_needs_no_clearing():
    """Packed genotypes of at most 32 bits: the likelihood caches are not cleared between fits, their entries carry the fit's epoch
    (mchap_hip.hip g_cache_epoch).  A batch run on one data set, its input then overwritten IN PLACE with another data set of the
    same shape (same workspace, same cache tables, full of the first run's entries under the same keys) and run again: the traces of
    the second data set exactly, as from a fresh batch and as with the caches cleared per call (tuning flag 65536)."""
    import torch

    from mchap_amd import DenovoMCMC
    from mchap_amd.device import DenovoDeviceBatch
    from mchap_amd.synth import synth_units

    kw = dict(ploidy=4, n_pos=8, n_reads=40, qual=(3, 20))        # chains that keep moving: thousands of cache entries each
    a, _, _ = synth_units(64, first_unit=0, **kw)
    b, _, _ = synth_units(64, first_unit=500, **kw)
    model = DenovoMCMC(ploidy=4, n_alleles=[2] * 8, steps=300, chains=2, random_seed=11)
    for kernel in (5, 3):
        m = DenovoMCMC(ploidy=4, n_alleles=[2] * 8, steps=300, chains=2, random_seed=11, kernel=kernel)
        fresh = DenovoDeviceBatch(m, b)
        fresh.run()
        reused = DenovoDeviceBatch(m, a)
        reused.run()
        torch.cuda.synchronize()
        first = reused.d_trace.clone()
        reused.d_reads.copy_(torch.from_numpy(np.ascontiguousarray(b).reshape(-1)).to(reused.d_reads.device))
        reused.run()
        torch.cuda.synchronize()
        assert not torch.equal(first, reused.d_trace)
        assert torch.equal(fresh.d_trace, reused.d_trace) and torch.equal(fresh.d_llks.view(torch.int64), reused.d_llks.view(torch.int64))
        os.environ["MCHAP_HIP_FLAGS"] = "65536"
        try:
            cleared = DenovoDeviceBatch(m, b)
            cleared.run()
            torch.cuda.synchronize()
        finally:
            os.environ.pop("MCHAP_HIP_FLAGS", None)
        assert torch.equal(cleared.d_trace, reused.d_trace)


def test_two_library_copies_never_tag_different_data_alike():
    """The likelihood caches of packed genotypes are not cleared between fits: an entry carries the epoch of the fit that wrote it.
    Until round 5 every loaded copy of the library counted its own epochs from 1 -- and the parity suite loads libmchap_hip.so and
    libmchap_hip_test.so side by side while torch's allocator hands the same workspace block to both: the first fit of the second
    copy then found the first copy's entries under its own epoch.  Now the epoch is a property of the call
    (mchap_denovo_cfg.cache_epoch, one sequence per process: mchap_amd/_lib.py next_cache_epoch).  A fresh process: copy A fits
    units X, its buffers go back to the allocator, copy B fits units Y of the same shape in the same block -- and must give what it
    gives with the caches cleared (flag 65536)."""
    import os
    import subprocess
    import sys

    code = r'''
import os, sys
import numpy as np
import torch
from mchap_amd import DenovoMCMC, _lib
from mchap_amd.device import DenovoDeviceBatch
from mchap_amd.synth import synth_units

kw = dict(ploidy=4, n_alleles=[2] * 8, steps=200, chains=2, random_seed=3)
X, _, _ = synth_units(300, ploidy=4, n_pos=8, n_reads=40, qual=(3, 20), first_unit=0)
Y, _, _ = synth_units(300, ploidy=4, n_pos=8, n_reads=40, qual=(3, 20), first_unit=5000)
os.environ.pop("MCHAP_HIP_TEST_KERNELS", None)
a = DenovoDeviceBatch(DenovoMCMC(**kw), X)
a.run(); torch.cuda.synchronize()
ptr_a = a.d_ws.data_ptr()
del a
os.environ["MCHAP_HIP_TEST_KERNELS"] = "1"
b = DenovoDeviceBatch(DenovoMCMC(**kw), Y)
same_block = b.d_ws.data_ptr() == ptr_a
b.run(); torch.cuda.synchronize()
wb = b.traces()[0].copy(); lb = b.traces()[2].copy()
os.environ["MCHAP_HIP_FLAGS"] = "65536"
c = DenovoDeviceBatch(DenovoMCMC(**kw), Y)
c.run(); torch.cuda.synchronize()
wc, lc = c.traces()[0], c.traces()[2]
assert len(_lib._libs) == 2, list(_lib._libs)
print("same_block", same_block, "equal", bool(np.array_equal(wb, wc) and np.array_equal(lb, lc)))
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MCHAP_HIP_")}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "equal True" in out.stdout, out.stdout[-500:]
    assert "same_block True" in out.stdout, out.stdout[-500:]  # (the scenario did arise: the allocator recycled the block)
