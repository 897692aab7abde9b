"""Driver and differential fuzz of the trace-summary kernels (trace_posterior_kernel<8|32>, trace_incongruence_kernel<8|32> behind
the mchap_trace_* / mchap_call_incongruence_* entry points) against the plain definition of tests/trace_summary_reference.py.
run_launch makes a batch call and a listed call over a tests.trace_summary_cases.Launch, twice, and check_launch compares every
unit of both; draw_launch builds random-walk traces over small haplotype pools in every form.  tests/test_gpu_trace_summary_kernels.py
runs its cases through the same two functions.  Needs a GPU.  python tests/fuzz_trace_summary.py [launches] [seed]"""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import trace_summary_reference as ref  # noqa: E402
from tests.trace_summary_cases import Form, Launch  # noqa: E402

INT32_MIN = -2 ** 31
SENTINEL = 0x5A


def max_cap(L, ploidy_max, wph):
    L.mchap_trace_posterior_max_states_wph.restype = C.c_int
    return int(L.mchap_trace_posterior_max_states_wph(ploidy_max, wph))


def batch_cap(L, launch):
    return min(512, max_cap(L, launch.ploidy_max, launch.form.W))


def listed_cap(L, launch):
    return launch.cap if launch.cap is not None else min(launch.n_obs, max_cap(L, launch.ploidy_max, launch.form.W))


def pack_launch(launch):
    """(units [U] of _lib.UNIT_DTYPE, the traces' words int64 [*]): unit u's trace at trace_off = the words before it."""
    from mchap_amd import _lib

    f = launch.form
    units = np.zeros(len(launch.units), dtype=_lib.UNIT_DTYPE)
    parts, off = [], 0
    for u, (K, chs) in enumerate(launch.units):
        w = ref.pack_alleles(chs) if f.calling else ref.pack_trace(chs, f.W).view(np.int64)
        assert w.shape == (launch.chains, launch.steps, K * f.W)
        units[u]["ploidy"], units[u]["trace_off"] = K, off
        parts.append(w.reshape(-1))
        off += w.size
    return units, np.concatenate(parts)


def _once(L, launch):
    """The batch call over every unit, then the listed call over launch.unit_list: a dict of host arrays of both."""
    import torch

    from mchap_amd import _lib

    f = launch.form
    U, W, pm = len(launch.units), f.W, launch.ploidy_max
    KW = pm * W
    units, words = pack_launch(launch)
    d_units = torch.from_numpy(units.view(np.uint8).reshape(-1).copy()).cuda()
    d_trace = torch.from_numpy(words).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    steps, chains, burn, ms = launch.steps, launch.chains, launch.burn, launch.max_states
    thr = C.c_double(launch.threshold)

    def buf(n, dtype):
        t = torch.empty(n, dtype=dtype, device="cuda")
        t.view(torch.uint8).fill_(SENTINEL)
        return t

    d = dict(words=buf(U * ms * KW, torch.int64), counts=buf(U * ms, torch.int32), n=buf(U, torch.int32), stats=buf(U * 2, torch.float64),
             mode=buf(U, torch.int32), mw=buf(U * KW, torch.int64), mc=buf(U, torch.int32), mci=buf(U, torch.int32))
    per_unit = (p(d["n"]), p(d["stats"]), p(d["mode"]), p(d["mw"]), p(d["mc"]), None)
    if W == 1:
        _lib.check(L.mchap_trace_posterior_batch_device(U, p(d_units), steps, chains, burn, p(d_trace), ms, pm, p(d["words"]), p(d["counts"]),
                                                        *per_unit))
    else:
        _lib.check(L.mchap_trace_posterior_batch_wph_device(U, p(d_units), steps, chains, burn, p(d_trace), ms, pm, W, p(d["words"]),
                                                            p(d["counts"]), *per_unit))
    if f.calling:
        _lib.check(L.mchap_call_incongruence_batch_device(U, p(d_units), steps, chains, burn, p(d_trace), pm, thr, p(d["mci"]), None))
    elif W == 1:
        _lib.check(L.mchap_trace_incongruence_batch_device(U, p(d_units), steps, chains, burn, p(d_trace), pm, thr, p(d["mci"]), None))
    else:
        _lib.check(L.mchap_trace_incongruence_batch_wph_device(U, p(d_units), steps, chains, burn, p(d_trace), pm, W, thr, p(d["mci"]), None))
    torch.cuda.synchronize()

    def host(per_state_rows, rows):
        return dict(words=d["words"].cpu().numpy().view(np.uint64).reshape(per_state_rows, rows, KW).copy(),
                    counts=d["counts"].cpu().numpy().reshape(per_state_rows, rows).copy(), n=d["n"].cpu().numpy().copy(),
                    stats=d["stats"].cpu().numpy().reshape(U, 2).copy(), mode=d["mode"].cpu().numpy().copy(),
                    mw=d["mw"].cpu().numpy().view(np.uint64).reshape(U, KW).copy(), mc=d["mc"].cpu().numpy().copy(),
                    mci=d["mci"].cpu().numpy().copy())

    out = dict(batch=host(U, ms))
    lst = np.asarray(launch.unit_list, dtype=np.int32)
    cap = listed_cap(L, launch)
    assert 1 <= cap <= max_cap(L, pm, W) and len(lst) >= 1 and lst.min() >= 0 and lst.max() < U
    d_list = torch.from_numpy(lst).cuda()
    d["words"], d["counts"] = buf(len(lst) * cap * KW, torch.int64), buf(len(lst) * cap, torch.int32)
    if W == 1:
        _lib.check(L.mchap_trace_posterior_listed_device(len(lst), p(d_list), p(d_units), steps, chains, burn, p(d_trace), cap, pm, p(d["words"]),
                                                         p(d["counts"]), *per_unit))
    else:
        _lib.check(L.mchap_trace_posterior_listed_wph_device(len(lst), p(d_list), p(d_units), steps, chains, burn, p(d_trace), cap, pm, W,
                                                             p(d["words"]), p(d["counts"]), *per_unit))
    if f.calling:
        _lib.check(L.mchap_call_incongruence_listed_device(len(lst), p(d_list), p(d_units), steps, chains, burn, p(d_trace), cap, pm, thr,
                                                           p(d["mci"]), None))
    elif W == 1:
        _lib.check(L.mchap_trace_incongruence_listed_device(len(lst), p(d_list), p(d_units), steps, chains, burn, p(d_trace), cap, pm, thr,
                                                            p(d["mci"]), None))
    else:
        _lib.check(L.mchap_trace_incongruence_listed_wph_device(len(lst), p(d_list), p(d_units), steps, chains, burn, p(d_trace), cap, pm, W,
                                                                thr, p(d["mci"]), None))
    torch.cuda.synchronize()
    out["listed"] = host(len(lst), cap)
    return out


def run_launch(L, launch):
    """Both calls, made twice from fresh buffers: the two runs' outputs are bit-equal (every buffer whole, untouched rows
    included)."""
    a, b = _once(L, launch), _once(L, launch)
    for call in ("batch", "listed"):
        for k in a[call]:
            assert a[call][k].tobytes() == b[call][k].tobytes(), (launch.name, launch.form.id, call, k)
    return a


def _padded(state, f, KW):
    w = list(state) if f.calling else ref.pack_state(state, f.W)
    return np.array(w + [0] * (KW - len(w)), dtype=np.uint64)


def _check_unit(launch, u, got, row, cap, rows, where, seen):
    """Unit u of one call against the definition.  got: the call's host arrays; row: the unit's row of the per-state outputs.
    Returns the SPM's deviation from the exact sum as a fraction of its bound (None where there is no SPM)."""
    f = launch.form
    K = launch.units[u][0]
    KW = launch.ploidy_max * f.W
    chains = launch.burnt(u)
    if K > launch.ploidy_max:   # refused: the tables are sized for ploidy_max
        assert got["n"][u] == INT32_MIN and np.isnan(got["stats"][u]).all() and got["mode"][u] == -1 and got["mc"][u] == 0, where
        assert got["mci"][u] == -1, where
        return None
    # incongruence: -1 when a chain alone visits more states than the table holds
    if max(ref.distinct_count([c]) for c in chains) > cap:
        assert got["mci"][u] == -1, where
    else:
        want = (ref.incongruence_calling if f.calling else ref.incongruence_denovo)(chains, launch.threshold)
        assert got["mci"][u] == want, (where, int(got["mci"][u]), want)
        if u in launch.codes:
            assert want == launch.codes[u], (where, want, launch.codes[u])
        seen.add(int(want))
    R = ref.posterior(chains)
    d = len(R.states)
    if d > cap:   # overflow: the sign is what callers use; -post_n bounds the distinct states from above
        assert got["n"][u] < 0 and got["n"][u] != INT32_MIN and -int(got["n"][u]) >= d, (where, int(got["n"][u]), d)
        assert -int(got["n"][u]) <= launch.n_obs, where
        # ... and the table itself is whole: the first `cap` distinct states, each with every one of its occurrences
        states, counts = ref.overflowed_table(chains, cap)
        shown = min(cap, rows)
        for r in range(shown):
            assert np.array_equal(got["words"][row, r], _padded(states[r], f, KW)), (where, "overflowed, rank", r)
        assert got["counts"][row, :shown].tolist() == counts[:shown], (where, "overflowed")
        return None
    assert got["n"][u] == d, (where, int(got["n"][u]), d)
    shown = min(d, rows)
    for r in range(shown):
        assert np.array_equal(got["words"][row, r], _padded(R.states[r], f, KW)), (where, "rank", r)
    assert got["counts"][row, :shown].tolist() == R.counts[:shown], where
    assert not got["words"][row, shown:].any() and not got["counts"][row, shown:].any(), where   # (d < rows: zero rows)
    assert got["mode"][u] == R.mode_index and got["mc"][u] == R.mode_count, (where, int(got["mode"][u]), R.mode_index)
    assert np.array_equal(got["mw"][u], _padded(R.mode_state, f, KW)), where
    assert got["stats"][u, 1] == R.gpm, (where, got["stats"][u, 1], R.gpm)
    spm = float(got["stats"][u, 0])
    assert np.isfinite(spm), where
    dev = abs(Fraction(spm) - R.spm_exact)
    bound = Fraction(ref.spm_bound(R.support_size))
    assert dev <= bound, (where, spm, float(R.spm_exact), float(dev), float(bound))
    return float(dev / bound)


def check_launch(L, launch, out):
    """Every unit of the batch call, every listed unit of the listed call (per-state outputs by list position, per-unit outputs by
    unit), and the bits of the units the list leaves out.  Returns (worst SPM deviation as a fraction of its bound, the MCI codes
    produced)."""
    worst, seen = 0.0, set()
    U = len(launch.units)
    tag = "%s %s" % (launch.name, launch.form.id)
    for u in range(U):
        dev = _check_unit(launch, u, out["batch"], u, batch_cap(L, launch), launch.max_states, "%s batch unit %d" % (tag, u), seen)
        worst = max(worst, dev or 0.0)
    cap = listed_cap(L, launch)
    for i, u in enumerate(launch.unit_list):
        dev = _check_unit(launch, u, out["listed"], i, cap, cap, "%s listed[%d] unit %d" % (tag, i, u), seen)
        worst = max(worst, dev or 0.0)
    for u in set(range(U)) - set(launch.unit_list):
        for k in ("n", "stats", "mode", "mw", "mc", "mci"):
            assert out["listed"][k][u].tobytes() == out["batch"][k][u].tobytes(), (tag, "unlisted unit", u, k)
    return worst, seen


# ---- the fuzz: random walks over small haplotype pools ----
def _pool(rng, kind, size):
    if kind == "call":
        return [int(a) for a in rng.choice(40, size=size, replace=False)]
    if kind == "w1":
        return [int(h) for h in {int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)) for _ in range(size)} | {0}][:size]
    # two words: high words from two values, low words from three, so about half of the pairs of haplotypes share one word
    his = [0, int(rng.integers(0, 2 ** 63)) * 2 + 1]
    los = [0] + [int(rng.integers(0, 2 ** 63)) * 2 + 1 for _ in range(2)]
    pairs = [(h << 64) | l for h in his for l in los]
    return [pairs[i] for i in rng.permutation(len(pairs))[:size]]


def draw_launch(rng, index=0):
    kind = ("w1", "w2", "call")[index % 3]   # the forms in turn
    pm = int(rng.integers(1, 16 if kind == "w2" else 9))
    f = Form(kind, pm)
    chains, steps = int(rng.integers(1, 5)), int(rng.integers(2, 120))
    burn = int(rng.integers(0, steps))
    units = []
    for _ in range(int(rng.integers(4, 6))):
        K = pm if rng.random() < 0.5 else int(rng.integers(1, pm + 1))
        pool = _pool(rng, kind, int(rng.integers(2, 6)))
        move = float(rng.choice([0.02, 0.1, 0.5]))
        chs = []
        for _c in range(chains):
            cur = [pool[int(i)] for i in rng.integers(0, len(pool), size=K)]
            if rng.random() < 0.5 and chs:
                cur = list(chs[0][-1])   # start where the first chain ended: chains that agree
            chain = []
            for _s in range(steps):
                if rng.random() < move:
                    cur = list(cur)
                    cur[int(rng.integers(0, K))] = pool[int(rng.integers(0, len(pool)))]
                chain.append(tuple(sorted(cur)))
            chs.append(chain)
        units.append((K, chs))
    U = len(units)
    n_list = int(rng.integers(1, U + 1))
    return Launch("fuzz %d" % index, f, units, steps, chains, burn, threshold=float(rng.choice([0.3, 0.5, 0.6, 0.9])), ploidy_max=pm,
                  max_states=int(rng.integers(1, 13)), cap=int(rng.choice([3, 8, 40, 200])),
                  unit_list=[int(u) for u in rng.permutation(U)[:n_list]])


def drawn(n_launches, seed):
    rng = np.random.default_rng(seed)
    for i in range(n_launches):
        yield draw_launch(np.random.default_rng(int(rng.integers(0, 2 ** 31))), i)


def run(n_launches, seed):
    """n_launches random launches through run_launch / check_launch; returns (units, worst SPM deviation / bound, codes seen)."""
    from mchap_amd import _lib

    L = _lib.lib()
    units, worst, seen = 0, 0.0, set()
    for launch in drawn(n_launches, seed):
        w, s = check_launch(L, launch, run_launch(L, launch))
        units += len(launch.units)
        worst, seen = max(worst, w), seen | s
        print("%s: %s, %d units, ploidy_max %d, %d chains x %d steps, burn %d: SPM within %.3g of its bound" % (
            launch.name, launch.form.kind, len(launch.units), launch.ploidy_max, launch.chains, launch.steps, launch.burn, w), flush=True)
    print("fuzz_trace_summary: %d launches, %d units, seed %d: codes %s" % (n_launches, units, seed, sorted(seen)), flush=True)
    return units, worst, seen


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 40, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
