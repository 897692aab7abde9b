"""The de novo host's two decisions -- which sampler a batch runs on and how many bytes of workspace it asks for -- over a table
of shapes, under both libraries, against values recorded before the decisions were gathered into one function
(tests/golden/denovo_sizing.json).  No compute calls: the library loads without a device, the budgets are then their caps.

Every case keeps n_units * chains <= 8: 65 536 cache slots and 64 context slots per chain stay under 512 MB, so a device with
4 GB free (an eighth of it is a budget's limit) gives what no device gives.

`python -m tests.test_denovo_sizing` rewrites the golden file from the libraries as built."""
import ctypes as C
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denovo_sizing.json")
LIBRARIES = {"libmchap_hip": "", "libmchap_hip_test": "1"}

# name: (units as (ploidy, SNVs, alleles, reads) each, DenovoMCMC keywords, tuning fields, pass the units)
A = [(4, 8, 2, 200)] * 4
CASES = {
    "a-k4-8snvs-200reads": (A, {}, {}, True),
    "b-20reads": ([(4, 8, 2, 20)] * 4, {}, {}, True),
    "c-k8-20snvs-1000reads-4chains": ([(8, 20, 2, 1000)] * 2, dict(chains=4), {}, True),
    "d-k4-6snvs-2600reads": ([(4, 6, 2, 2600)] * 4, {}, {}, True),
    "e-k4-12snvs-3alleles": ([(4, 12, 3, 200)] * 4, {}, {}, True),
    "f-4temperatures": (A, dict(temperatures=(0.25, 0.5, 0.75, 1.0)), {}, True),
    "g-kernel3": (A, dict(kernel=3), {}, True),
    "h-kernel2-k3": ([(3, 8, 2, 200)] * 4, dict(kernel=2), {}, True),
    "i-ploidies-2-and-4": ([(2, 8, 2, 200), (4, 8, 2, 200)] * 2, {}, {}, True),
    "j-70snvs": ([(4, 70, 2, 200)] * 4, {}, {}, True),
    "k-ploidy12": ([(12, 8, 2, 200)] * 4, {}, {}, True),
    "l-k4-50snvs": ([(4, 50, 2, 200)] * 4, {}, {}, True),
    "m-cache-off": (A, dict(llk_cache_threshold=-1), {}, True),
    "n-cache-slots-256": (A, {}, dict(cache_slots=256), True),
    "o-no-contexts": (A, {}, dict(flags=524288), True),
    "p-kernel1": (A, dict(kernel=1), {}, True),
    "p-kernel1-no-units": (A, dict(kernel=1), {}, False),
    "q-kernel4": (A, dict(kernel=4), {}, True),
    "r-5000reads": ([(4, 8, 2, 5000)] * 4, {}, {}, True),
}


def measure(L, case):
    """What the library answers for one case: sampler name (with its return code, and the error text if it failed), trace words
    per haplotype, workspace bytes."""
    from mchap_amd import DenovoMCMC, _lib

    shapes, kw, tuning, with_units = CASES[case]
    units = np.zeros(len(shapes), dtype=_lib.UNIT_DTYPE)
    for u, (ploidy, n_pos, max_allele, n_reads) in zip(units, shapes):
        u["ploidy"], u["n_pos"], u["max_allele"], u["n_reads"] = ploidy, n_pos, max_allele, n_reads
    M = max(s[1] for s in shapes)
    model = DenovoMCMC(ploidy=shapes[0][0], n_alleles=[shapes[0][2]] * M, random_seed=1, **kw)
    cfg = model._cfg(M)
    assert len(shapes) * model.chains <= 8
    if tuning:
        t = _lib.DenovoTuning(**tuning)
        cfg._tuning = t
        cfg.tuning = C.pointer(t)
    up = _lib.ptr(units) if with_units else None
    buf = C.create_string_buffer(160)
    rc = L.mchap_denovo_sampler_name(C.byref(cfg), len(units), up, buf, 160)
    return {
        "rc": rc,
        "error": L.mchap_last_error().decode() if rc else None,
        "sampler_name": buf.value.decode() if rc == 0 else None,
        "trace_words_per_haplotype": L.mchap_denovo_trace_words_per_haplotype(C.byref(cfg), len(units), up),
        "workspace_bytes": L.mchap_denovo_workspace_bytes(C.byref(cfg), len(units), up),
    }


def _library(monkeypatch, test_kernels):
    from mchap_amd import _lib

    for k in [k for k in os.environ if k.startswith("MCHAP_HIP_")]:  # (the tuning variables DenovoMCMC._cfg reads)
        monkeypatch.delenv(k)
    if test_kernels:
        monkeypatch.setenv("MCHAP_HIP_TEST_KERNELS", test_kernels)
    return _lib.lib()


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_sampler_plan_and_workspace_sizes_are_the_recorded_ones(library, monkeypatch):
    L = _library(monkeypatch, LIBRARIES[library])
    if L.mchap_device_count() > 0:
        import torch

        if torch.cuda.mem_get_info()[0] < 4 << 30:
            pytest.skip("a device is visible and reports less than 4 GB free: its budgets are below their caps")
    with open(GOLDEN) as f:
        golden = json.load(f)[library]
    assert sorted(golden) == sorted(CASES)
    got = {case: measure(L, case) for case in CASES}
    for case in CASES:
        assert got[case] == golden[case], case
    # the table does take the paths it is there for
    names = {c: got[c]["sampler_name"] for c in CASES}
    assert "phased" in names["a-k4-8snvs-200reads"] and "u128" in names["j-70snvs"] and "u128" in names["k-ploidy12"]
    assert got["j-70snvs"]["trace_words_per_haplotype"] == 2 and got["r-5000reads"]["rc"] != 0
    assert got["m-cache-off"]["workspace_bytes"] < got["n-cache-slots-256"]["workspace_bytes"] < got["a-k4-8snvs-200reads"]["workspace_bytes"]
    assert got["o-no-contexts"]["workspace_bytes"] < got["a-k4-8snvs-200reads"]["workspace_bytes"]


if __name__ == "__main__":
    from mchap_amd import _lib

    for k in [k for k in os.environ if k.startswith("MCHAP_HIP_")]:
        del os.environ[k]
    out = {}
    for library, test_kernels in LIBRARIES.items():
        if test_kernels:
            os.environ["MCHAP_HIP_TEST_KERNELS"] = test_kernels
        out[library] = {case: measure(_lib.lib(), case) for case in CASES}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
