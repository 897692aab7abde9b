"""The C-ABI library builds for gfx950, loads without a GPU and exports every symbol include/mchap_hip.h
declares.  No compute calls here."""
import os
import re

import pytest

from tests.conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "mchap_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mchap_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from mchap_amd import _lib

    _lib.build()
    L = _lib.lib()
    names = _declared()
    assert len(names) >= 10
    for n in names:
        assert hasattr(L, n), n
    assert sorted(_lib.EXPORTS) == names
    assert b"gfx950" in L.mchap_version()


def test_fails_loudly_without_gpu():
    from mchap_amd import DenovoMCMC, _lib
    from mchap_amd.synth import synth_units

    if _lib.lib().mchap_device_count() > 0:
        pytest.skip("a GPU is visible")
    reads, _, _ = synth_units(1, n_reads=10, n_pos=3)
    with pytest.raises(_lib.MchapLibraryError):
        DenovoMCMC(ploidy=4, n_alleles=[2, 2, 2], steps=5, random_seed=1).fit(reads[0])


def test_product_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/: neither the package nor
    the profiling tools do."""
    bad = []
    for top in ("mchap_amd", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".inc", ".sh")):
                    txt = open(os.path.join(dirpath, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "mchap_oracle" in txt or "libmchap_oracle" in txt:
                        bad.append(os.path.join(top, f))
    assert not bad, bad


def test_lds_and_workspace_sizing():
    import ctypes as C
    from mchap_amd import DenovoMCMC, _lib

    L = _lib.lib()
    # config #2: 8 SNVs x 2 alleles x 256 padded reads x 8 B = 32 KiB + per-chain scratch
    n = L.mchap_denovo_lds_bytes(200, 8, 2, 4, 2, 1)
    assert 32768 < n < 40000
    assert L.mchap_denovo_lds_bytes(200, 8, 2, 12, 2, 1) < 0
    cfg = DenovoMCMC(ploidy=4, n_alleles=[2] * 8, random_seed=1, kernel=1)._cfg(8)
    # the call's break table ((8 + 1) x 8 doubles, rounded to 256 B) + 1024 cache entries of 16 B per chain
    assert L.mchap_denovo_workspace_bytes(C.byref(cfg), 10, None) == 768 + 10 * 2 * 1024 * 16


def _null_buffer_calls(L):
    """One entry point of each host object of the library that reports errors, with one unit and NULL for a required buffer:
    (object, the call, the error text as the parent of the split into objects reported it).  Each returns before it touches the
    device."""
    import ctypes as C

    i64 = C.c_int64
    return [
        # mchap_exact_call_batch_device(n_units, reads, n_reads, n_pos, max_allele, read_counts, haplotypes, n_haps, ploidy, has_prior,
        #                               inbreeding, frequencies, out, workspace, workspace_bytes, stream)
        ("exact caller", lambda: L.mchap_exact_call_batch_device(1, None, 8, 3, 2, None, None, 4, 2, 0, None, None, None, None, i64(0), None),
         b"NULL buffer"),
        # mchap_call_mcmc_batch_device(n_units, reads, n_reads, n_pos, max_allele, read_counts, haplotypes, n_haps, ploidy, has_prior,
        #                              inbreeding, frequencies, initial, stream_ids, steps, chains, step_type, seed, genotypes, llks,
        #                              status, workspace, workspace_bytes, stream)
        ("call sampler", lambda: L.mchap_call_mcmc_batch_device(1, None, 8, 3, 2, None, None, 4, 2, 0, None, None, None, None, 50, 2, 0,
                                                                C.c_uint64(1), None, None, None, None, i64(0), None),
         b"NULL buffer"),
        # mchap_trace_posterior_batch_device(n_units, units, steps, chains, burn, trace_words, max_states, ploidy_max, post_words,
        #                                    post_counts, post_n, mode_stats, mode_index, mode_words, mode_count, stream)
        ("trace posterior", lambda: L.mchap_trace_posterior_batch_device(1, None, 10, 2, 0, None, 4, 4, None, None, None, None, None, None,
                                                                         None, None),
         b"NULL buffer"),
        # mchap_pileup_overlap_device(bytes, n_bytes, segments, first, n_segments, n_positions, stream)
        ("pileup", lambda: L.mchap_pileup_overlap_device(None, 0, None, None, 1, 1, None), b"pileup overlap: NULL buffer"),
    ]


def test_trace_summaries_refuse_on_the_host():
    """What launch_posterior / launch_incongruence (csrc/posterior_api.hip) turn away before the device is touched: every buffer is
    a non-NULL address that is never read."""
    import ctypes as C

    from mchap_amd import _lib

    L = _lib.lib()
    L.mchap_trace_posterior_max_states_wph.restype = C.c_int
    scratch = C.create_string_buffer(64)
    b = C.c_void_p(C.addressof(scratch))
    thr = C.c_double(0.6)

    def posterior(steps=10, chains=2, burn=0, ploidy_max=4, wph=1, cap=None):
        if cap is None:
            return L.mchap_trace_posterior_batch_wph_device(1, b, steps, chains, burn, b, 4, ploidy_max, wph, b, b, b, b, b, b, b, None)
        return L.mchap_trace_posterior_listed_wph_device(1, b, b, steps, chains, burn, b, cap, ploidy_max, wph, b, b, b, b, b, b, b, None)

    def incongruence(steps=10, chains=2, burn=0, ploidy_max=4, wph=1, cap=None):
        if cap is None:
            return L.mchap_trace_incongruence_batch_wph_device(1, b, steps, chains, burn, b, ploidy_max, wph, thr, b, None)
        return L.mchap_trace_incongruence_listed_wph_device(1, b, b, steps, chains, burn, b, cap, ploidy_max, wph, thr, b, None)

    for call in (posterior, incongruence):
        for burn in (10, 11, -1):
            assert call(burn=burn) == _lib.ERR_BAD_ARG and L.mchap_last_error() == b"burn must be in [0, steps)", (call.__name__, burn)
        assert call(wph=3) == _lib.ERR_LIMIT and L.mchap_last_error() == b"ploidy_max 4 at 3 word(s) per haplotype out of range"
        assert call(ploidy_max=9) == _lib.ERR_LIMIT and L.mchap_last_error() == b"ploidy_max 9 at 1 word(s) per haplotype out of range"
        assert call(ploidy_max=16, wph=2) == _lib.ERR_LIMIT
        for pm, wph in ((4, 1), (8, 1), (15, 2)):
            most = int(L.mchap_trace_posterior_max_states_wph(pm, wph))
            assert most >= 512
            assert call(ploidy_max=pm, wph=wph, cap=most + 1) == _lib.ERR_LIMIT
            assert (b"a table of %d states does not fit the LDS at ploidy %d (at most %d)" % (most + 1, pm, most)) == L.mchap_last_error()
    assert incongruence(cap=0) == _lib.ERR_LIMIT
    assert posterior(cap=0) == _lib.ERR_BAD_ARG and L.mchap_last_error() == b"max_states must be >= 1"   # (a listed call's rows are its table)
    assert L.mchap_trace_posterior_max_states_wph(9, 1) == 0 and L.mchap_trace_posterior_max_states_wph(4, 3) == 0
    assert incongruence(chains=33) == _lib.ERR_LIMIT and L.mchap_last_error() == b"chains must be in 1..32"
    assert incongruence(chains=0) == _lib.ERR_LIMIT
    # the calling form goes through the same checks
    assert L.mchap_call_incongruence_batch_device(1, b, 10, 33, 0, b, 4, thr, b, None) == _lib.ERR_LIMIT
    assert L.mchap_last_error() == b"chains must be in 1..32"
    assert L.mchap_call_incongruence_listed_device(1, b, b, 10, 2, 10, b, 70, 4, thr, b, None) == _lib.ERR_BAD_ARG
    assert L.mchap_call_incongruence_batch_device(1, b, 10, 2, 0, b, 9, thr, b, None) == _lib.ERR_LIMIT


@pytest.fixture(params=["", "1"], ids=["libmchap_hip", "libmchap_hip_test"])
def either_library(request, monkeypatch):
    from mchap_amd import _lib

    _lib.build()
    if request.param:
        monkeypatch.setenv("MCHAP_HIP_TEST_KERNELS", request.param)
    else:
        monkeypatch.delenv("MCHAP_HIP_TEST_KERNELS", raising=False)
    return _lib.lib()


def test_every_host_object_reports_through_the_one_error_buffer(either_library):
    """The exact caller, the call sampler, the trace summaries and the pileup are objects of their own; mchap_last_error reads one
    buffer per library, and each of them writes it.  Before each call the buffer holds another object's text."""
    import ctypes as C

    from mchap_amd import _lib

    L = either_library
    for name, call, text in _null_buffer_calls(L):
        if name == "pileup":  # (another object's error first: a unit list that is NULL, from the trace summaries)
            assert L.mchap_trace_posterior_listed_device(1, None, None, 10, 2, 0, None, 4, 4, None, None, None, None, None, None, None,
                                                         None) == _lib.ERR_BAD_ARG
            assert L.mchap_last_error() == b"NULL unit list"
        else:
            assert L.mchap_pileup_filter_device(None, None, 1, 0, 0.0, 0, 0.0, 0, 0, None, None, None) == _lib.ERR_BAD_ARG
            assert L.mchap_last_error() == b"pileup filter: NULL buffer or no samples"
        assert call() == _lib.ERR_BAD_ARG, name
        assert L.mchap_last_error() == text, name


def test_the_two_libraries_keep_their_error_texts_apart(monkeypatch):
    """libmchap_hip.so and libmchap_hip_test.so loaded in one process: an error raised through one leaves the other's
    mchap_last_error as it was, whichever object of either raised it."""
    from mchap_amd import _lib

    _lib.build()
    monkeypatch.delenv("MCHAP_HIP_TEST_KERNELS", raising=False)
    A = _lib.lib()
    monkeypatch.setenv("MCHAP_HIP_TEST_KERNELS", "1")
    B = _lib.lib()
    assert A is not B and A._name != B._name
    for first, second in ((A, B), (B, A)):
        for name, call, text in _null_buffer_calls(second):
            # `first` holds a text no call of _null_buffer_calls produces ...
            assert first.mchap_pileup_filter_device(None, None, 1, 0, 0.0, 0, 0.0, 0, 0, None, None, None) == _lib.ERR_BAD_ARG
            kept = b"pileup filter: NULL buffer or no samples"
            assert first.mchap_last_error() == kept
            # ... and keeps it while every object of `second` fails
            assert call() == _lib.ERR_BAD_ARG, name
            assert second.mchap_last_error() == text, name
            assert first.mchap_last_error() == kept, name
