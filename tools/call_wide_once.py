"""Measurement aid: one `mchap call` sampler call (mchap_call_mcmc_batch_device) at ploidy 4, 100 reads, 2000 steps x 2 chains and
1024 units over H known haplotypes, timed with HIP events (DESIGN.md "The call sampler over many known
haplotypes").

  python tools/call_wide_once.py H [runs] [units]        H <= 256: the default path, or call_wide_kernel under MCHAP_HIP_CALL_WIDE=1

The chains' tables of remembered likelihoods are sized for the worst case (2 x steps x ploidy x H entries of 16 bytes a chain:
134 MB at H = 512), so beyond H = 256 the 1024 units do not fit the HBM at once: the call is then cut into as many equal
sub-batches as 70 % of the free memory asks for, and a run's time is the sum over them.  One JSON line per invocation."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mchap_amd import _lib
from mchap_amd.synth import synth_units

H = int(sys.argv[1])
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
U = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
K, R, M, S, Cn = 4, 100, 12, 2000, 2

L = _lib.lib()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
rng = np.random.default_rng(H)
reads, _, truth = synth_units(U, ploidy=K, n_pos=M, n_reads=R, first_unit=1, window=(2, M))
weights = 1 << np.arange(M)
haps = np.zeros((U, H, M), np.int8)
for u in range(U):  # H distinct haplotypes, the unit's own among them
    mine = np.unique(truth[u].astype(np.int64) @ weights)
    codes = np.concatenate([mine, rng.permutation(np.setdiff1d(np.arange(2 ** M), mine))[: H - len(mine)]])
    rng.shuffle(codes)
    haps[u] = ((codes[:, None] >> np.arange(M)[None, :]) & 1).astype(np.int8)

ws1 = int(L.mchap_call_mcmc_workspace_bytes_for(1, R, H, K, S, Cn))
per_unit = ws1 + Cn * S * (K + 1) * 8 + R * M * 2 * 8 + H * M + 4096
free, _ = torch.cuda.mem_get_info()
parts = max(1, -(-U * per_unit // int(free * 0.7)))
step = -(-U // parts)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
d_reads = torch.from_numpy(reads).to(dev)
d_haps = torch.from_numpy(haps).to(dev)
d_F = torch.full((U,), 0.1, dtype=torch.float64, device=dev)
d_sid = torch.arange(U, dtype=torch.int64, device=dev)
n = min(step, U)
d_g = torch.empty(n * Cn * S * K, dtype=torch.int64, device=dev)
d_l = torch.empty(n * Cn * S, dtype=torch.float64, device=dev)
d_st = torch.empty(n, dtype=torch.int32, device=dev)
ws = int(L.mchap_call_mcmc_workspace_bytes_for(n, R, H, K, S, Cn))
d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
times, moved = [], None
for run in range(runs + 1):  # (the first run is the warm-up: module load, the kernels' first launch)
    total = 0.0
    for u0 in range(0, U, step):
        m = min(step, U - u0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.mchap_call_mcmc_batch_device(m, p(d_reads[u0:]), R, M, 2, None, p(d_haps[u0:]), H, K, 1, p(d_F[u0:]), None, None, p(d_sid[u0:]),
                                                  S, Cn, 0, C.c_uint64(7), p(d_g), p(d_l), p(d_st), p(d_ws), C.c_int64(ws), stream))
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        assert int(d_st[:m].abs().sum()) == 0
    if run:
        times.append(total)
g = d_g[: Cn * S * K].cpu().numpy().reshape(Cn, S, K)
print(json.dumps(dict(H=H, path="wide" if (H > 256 or os.environ.get("MCHAP_HIP_CALL_WIDE") == "1") else "default", units=U, ploidy=K, reads=R,
                      steps=S, chains=Cn, sub_batches=parts, ms=[round(t, 1) for t in times], ms_median=round(float(np.median(times)), 1),
                      workspace_gb=round(ws / 2 ** 30, 1), last_genotype=g[0, -1].tolist())), flush=True)
