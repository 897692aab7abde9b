"""Device-resident batches: inputs and outputs stay in HBM, kernels are enqueued on the caller's
torch stream through the `*_device` entry points of the C ABI.  torch is used for device memory,
streams and (in bench.py) torch.distributed only.
"""
import ctypes as C
from math import comb

import numpy as np

from . import _lib
from .assemble import DenovoMCMC, unpack_trace


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise _lib.MchapLibraryError("no MI355X visible to torch: the device path needs a GPU (no CPU fallback)")
    return torch


def _ptr(t):
    """Torch tensor `t` as the C ABI takes a device buffer (None: NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _device(torch, device):
    """`device`, by default torch's current GPU."""
    return torch.device("cuda", torch.cuda.current_device()) if device is None else device


def pinned(a):
    """A copy of numpy array `a` in page-locked host memory (as a numpy array): uploads from it are asynchronous."""
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


class PassesInFlight:
    """Round-robin issue of whole passes (one device batch each: prepare pass, sampler, posterior summary) over
    `n` HIP streams.  A pass is a few dozen launches and several of them occupy a fraction of the chip (the prepare
    pass, the hand-back rounds of the phased sampler, every launch's last wave round); with three or four passes in
    flight those phases overlap the first phase of the next pass: 13.8 -> 10.6 ms per pass at 10 000 tetraploid loci
    (DESIGN.md 6).  Each pass needs device buffers of its own (its DenovoDeviceBatch / DenovoRaggedBatch).  The HIP
    runtime shares GPU_MAX_HW_QUEUES (default 4) hardware queues among a process's streams: export
    GPU_MAX_HW_QUEUES=8 (or 16) before the process touches the GPU so that four streams and the null stream get one each.

        flight = PassesInFlight(4)
        for batch in batches:
            flight.submit(lambda b=batch: (b.run(), b.posterior(burn)))
        flight.join()            # torch's current stream then waits for every pass
    """

    def __init__(self, n=4):
        torch = _torch()
        self.torch = torch
        self.streams = [torch.cuda.Stream() for _ in range(max(1, int(n)))]
        self.issued = 0

    def submit(self, enqueue):
        """Call `enqueue()` with the next stream current; what it enqueues starts after the work already on torch's
        current stream (inputs uploaded there are seen)."""
        s = self.streams[self.issued % len(self.streams)]
        self.issued += 1
        s.wait_stream(self.torch.cuda.current_stream())
        with self.torch.cuda.stream(s):
            return enqueue()

    def join(self):
        cur = self.torch.cuda.current_stream()
        for s in self.streams:
            cur.wait_stream(s)


class _OwnBuffers:
    """A device batch owns its buffers (inputs, workspace, traces, summaries): two passes over it must not overlap, whatever
    streams they are issued on.  Every enqueueing method waits for the event the previous one left behind and leaves its
    own -- passes of ONE batch are serialised on the device, passes of different batches still run side by side
    (PassesInFlight).

    The base of the de novo batches also sets those buffers up and launches the sampler over them: a batch builds its unit
    descriptors and input tensors (d_reads, or the compact input through _upload_compact), then _allocate; _fit is the launch."""

    _last_use = None
    _two_words = True   # the batch takes units of two trace words per haplotype (the general sampler's)
    d_reads = d_calls = d_quals = d_qual_prob = None

    def _begin(self):
        s = self.torch.cuda.current_stream()
        if self._last_use is not None:
            s.wait_event(self._last_use)
        return s

    def _end(self):
        ev = self.torch.cuda.Event()
        ev.record(self.torch.cuda.current_stream())
        self._last_use = ev

    def _allocate(self, desc, trace_words, llks, fixed):
        """Descriptors `desc` (their trace_off in words of a one-word batch) to the device, the outputs -- trace_words int64 (times
        the words per haplotype), llks float64, fixed int8, a status per unit -- and the workspace; sets cfg from self.max_pos."""
        torch, dev, L = self.torch, self.device, _lib.lib()
        U = len(desc)
        self.units_host, self.n_units = desc, U
        self.cfg = self.model._cfg(self.max_pos)
        # uint64 words per haplotype of the traces: 2 when the batch holds a unit of more than 62 SNVs / 64 bits per haplotype
        self.wph = int(L.mchap_denovo_trace_words_per_haplotype(C.byref(self.cfg), U, _lib.ptr(desc)))
        if self.wph < 1:
            raise NotImplementedError("mchap_hip: unsupported unit shape (" + _lib.last_error() + ")")
        if self.wph > 1 and not self._two_words:
            raise NotImplementedError("DenovoDeviceBatch holds one trace word per haplotype: units wider than 62 SNVs / 64 bits go "
                                      "through DenovoMCMC.fit_batch or DenovoRaggedBatch")
        desc["trace_off"] *= self.wph
        self.d_units = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(dev)
        self.d_trace = torch.empty(int(trace_words) * self.wph, dtype=torch.int64, device=dev)
        self.d_llks = torch.empty(int(llks), dtype=torch.float64, device=dev)
        self.d_fixed = torch.empty(int(fixed), dtype=torch.int8, device=dev)
        self.d_status = torch.empty(U, dtype=torch.int32, device=dev)
        self.ws_bytes = int(L.mchap_denovo_workspace_bytes(C.byref(self.cfg), U, _lib.ptr(desc)))
        if self.ws_bytes < 0:
            raise NotImplementedError("mchap_hip: unsupported unit shape")
        self.d_ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=dev)

    def _upload_compact(self, calls, quals, error_rate, non_blocking=False, reject_negative=None):
        """The compact input in place of d_reads: int8 calls (< 0 = gap), optional int16 quals of the same shape, and the table
        a called cell's quality is looked up in (one entry without qualities).  reject_negative: the name under which a called
        cell of negative quality is refused."""
        from .blockpath import qual_prob_table

        torch, dev = self.torch, self.device
        calls = np.ascontiguousarray(calls, dtype=np.int8)
        self.d_reads = None
        self.d_calls = torch.from_numpy(calls.reshape(-1)).to(dev, non_blocking=non_blocking)
        table = np.array([1.0 - error_rate], dtype=np.float64)   # qualities ignored: every called cell's probability
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.int16)
            assert quals.shape == calls.shape
            if reject_negative and (quals[calls >= 0] < 0).any():
                raise AssertionError(reject_negative + ": a called cell has a negative quality")
            self.d_quals = torch.from_numpy(quals.reshape(-1)).to(dev, non_blocking=non_blocking)
            table = qual_prob_table(error_rate, int(quals.max(initial=0)) + 1)   # reference io/bam.py:280-288
        self.qual_prob_len = len(table)
        self.d_qual_prob = torch.from_numpy(table).to(dev)

    def _fit(self, stream):
        """The sampler launch on `stream` (a raw hipStream_t): from the float64 read tensors, or -- d_reads is None -- from the
        compact input, the tensors formed on the device by the prepare pass (mchap_denovo_fit_batch_calls_device)."""
        L = _lib.lib()
        self.cfg.cache_epoch = _lib.next_cache_epoch()  # (the call's own: one sequence for every library copy of the process)
        head = (C.byref(self.cfg), self.n_units, _ptr(self.d_units), _lib.ptr(self.units_host))
        tail = (_ptr(self.d_counts), _ptr(self.d_nalleles), None, _ptr(self.d_trace), _ptr(self.d_llks), _ptr(self.d_fixed),
                _ptr(self.d_status), _ptr(self.d_ws), C.c_int64(self.ws_bytes), C.c_void_p(stream))
        if self.d_reads is None:
            rc = L.mchap_denovo_fit_batch_calls_device(*head, _ptr(self.d_calls), _ptr(self.d_quals), _ptr(self.d_qual_prob),
                                                       int(self.qual_prob_len), *tail)
        else:
            rc = L.mchap_denovo_fit_batch_device(*head, _ptr(self.d_reads), *tail)
        _lib.check(rc)


class DenovoDeviceBatch(_OwnBuffers):
    """A batch of uniformly shaped units resident on one GPU.

    reads : float64 [U, R, M, A] (numpy, copied once) ; read_counts : int64 [U, R] or None."""

    _two_words = False   # (posterior / traces hold one word per haplotype)

    def __init__(self, model: DenovoMCMC, reads, read_counts=None, first_stream=0, device=None, calls=None, quals=None,
                 error_rate=0.0024):
        """reads: float64 [U, R, M, A]; or reads=None with calls int8 [U, R, M] (< 0 = gap), optional quals int16 of the
        same shape and the base error rate: the compact form the reference's encoders start from, turned into the
        probability tensor on the device (5x fewer bytes to upload, same traces).  The input arrays are copied on torch's
        current stream; when they live in page-locked host memory (mchap_amd.device.pinned) the copy does not block the
        host, and the caller keeps them unchanged until the stream has passed it."""
        torch = _torch()
        self.torch = torch
        self.model = model
        self.device = _device(torch, device)
        if reads is None:
            calls = np.ascontiguousarray(calls, dtype=np.int8)
            U, R, M = calls.shape
            A = int(np.max(model.n_alleles))
        else:
            reads = np.ascontiguousarray(reads, dtype=np.float64)
            U, R, M, A = reads.shape
        self.shape = (U, R, M, A)
        K, Cn, S = int(model.ploidy), int(model.chains), int(model.steps)
        self.K, self.Cn, self.S = K, Cn, S
        units = np.zeros(U, dtype=_lib.UNIT_DTYPE)
        idx = np.arange(U, dtype=np.int64)
        units["reads_off"] = idx * (R * M * A) if reads is not None else idx * (R * M)
        units["counts_off"] = idx * R if read_counts is not None else -1
        units["nalleles_off"] = 0
        units["initial_off"] = -1
        units["trace_off"] = idx * (Cn * S * K)
        units["llk_off"] = idx * (Cn * S)
        units["fixed_off"] = idx * M
        units["n_reads"], units["n_pos"], units["max_allele"], units["ploidy"] = R, M, A, K
        units["inbreeding"] = np.nan if model.inbreeding is None else float(model.inbreeding)
        units["stream_id"] = (first_stream + idx).astype(np.uint64)
        dev = self.device
        if reads is not None:
            self.d_reads = torch.from_numpy(reads.reshape(-1)).to(dev, non_blocking=True)
        else:
            # (unlike DenovoRaggedBatch.from_calls, a called cell of negative quality is not refused here)
            self._upload_compact(calls, quals, error_rate, non_blocking=True)
        self.d_counts = None if read_counts is None else torch.from_numpy(np.ascontiguousarray(read_counts, dtype=np.int64).reshape(-1)).to(dev)
        self.d_nalleles = torch.from_numpy(np.asarray(model.n_alleles, dtype=np.int8)).to(dev)
        self.max_pos = M
        self._allocate(units, U * Cn * S * K, U * Cn * S, U * M)
        self.post = None
        self.sampler_name = _lib.sampler_name(self.cfg, units)
        self.timer = None

    def time_sampler(self, on=True):
        """Bracket the sampler launches of every run() with HIP events on its stream; `sampler_ms()` reads the last span."""
        if on and self.timer is None:
            self.timer = _lib.SamplerTimer()
        self.cfg.timer = self.timer.handle if (on and self.timer is not None) else None

    def sampler_ms(self):
        return -1.0 if self.timer is None else self.timer.ms()

    def run(self):
        """Enqueue the sampler on torch's current stream (no synchronisation)."""
        self._fit(self._begin().cuda_stream)
        self._end()

    def posterior(self, burn, max_states=32):
        """Enqueue the posterior summary of the traces written by run()."""
        torch = self.torch
        U = self.shape[0]
        if self.post is None or self.post["max_states"] != max_states:
            dev = self.device
            self.post = dict(
                max_states=max_states,
                words=torch.empty(U * max_states * self.K, dtype=torch.int64, device=dev),
                counts=torch.empty(U * max_states, dtype=torch.int32, device=dev),
                n=torch.empty(U, dtype=torch.int32, device=dev),
                stats=torch.empty(U * 2, dtype=torch.float64, device=dev),
                mode=torch.empty(U, dtype=torch.int32, device=dev),
                mode_words=torch.empty(U * self.K, dtype=torch.int64, device=dev),
                mode_count=torch.empty(U, dtype=torch.int32, device=dev),
            )
        P = self.post
        stream = self._begin().cuda_stream
        rc = _lib.lib().mchap_trace_posterior_batch_device(
            U, _ptr(self.d_units), self.S, self.Cn, int(burn), _ptr(self.d_trace), int(max_states), self.K,
            _ptr(P["words"]), _ptr(P["counts"]), _ptr(P["n"]), _ptr(P["stats"]), _ptr(P["mode"]),
            _ptr(P["mode_words"]), _ptr(P["mode_count"]), C.c_void_p(stream))
        _lib.check(rc)
        self._end()

    def incongruence(self, burn, threshold=0.6):
        """Enqueue the replicate-incongruence code (MCI) of every unit's chains; returns the int32 device tensor
        (0 none, 1 incongruence, 2 putative CNV; reference GenotypeMultiTrace.replicate_incongruence)."""
        torch = self.torch
        U = self.shape[0]
        if getattr(self, "d_mci", None) is None:
            self.d_mci = torch.empty(U, dtype=torch.int32, device=self.device)
        stream = self._begin().cuda_stream
        rc = _lib.lib().mchap_trace_incongruence_batch_device(
            U, _ptr(self.d_units), self.S, self.Cn, int(burn), _ptr(self.d_trace), self.K, C.c_double(float(threshold)),
            _ptr(self.d_mci), C.c_void_p(stream))
        _lib.check(rc)
        self._end()
        return self.d_mci

    # ---- results back on the host ----
    def traces(self):
        U, R, M, A = self.shape
        w = self.d_trace.cpu().numpy().view(np.uint64).reshape(U, self.Cn, self.S, self.K)
        fixed = self.d_fixed.cpu().numpy().reshape(U, M)
        llks = self.d_llks.cpu().numpy().reshape(U, self.Cn, self.S)
        status = self.d_status.cpu().numpy()
        return w, fixed, llks, status

    def genotypes(self, u, words=None, fixed=None):
        if words is None:
            words, fixed, _, _ = self.traces()
        return unpack_trace(words[u], fixed[u], self.shape[3])

    def posterior_host(self):
        P = self.post
        U = self.shape[0]
        ms = P["max_states"]
        n = P["n"].cpu().numpy()
        if (n < 0).any():
            # more distinct genotypes than the kernel keeps (counts were dropped): the summary is not the posterior
            raise _lib.MchapLibraryError(
                "posterior summary overflow in %d unit(s): more than 512 distinct genotypes after burn-in; "
                "summarise those units from traces() instead" % int((n < 0).sum()))
        return dict(
            words=P["words"].cpu().numpy().view(np.uint64).reshape(U, ms, self.K),
            counts=P["counts"].cpu().numpy().reshape(U, ms),
            n=n,
            stats=P["stats"].cpu().numpy().reshape(U, 2),
            mode=P["mode"].cpu().numpy(),
            mode_words=P["mode_words"].cpu().numpy().view(np.uint64).reshape(U, self.K),
            mode_count=P["mode_count"].cpu().numpy(),
        )


def call_reads_from_calls(calls, counts, unit_rows, unit_call_off, unit_count_off, n_alleles, n_reads, max_allele, error_rate=0.0024,
                          device=None):
    """The read tensors of a shape group of `mchap call` / `mchap call-exact`, formed on the device from the compact arrays of
    blockpath.call_unit_inputs (mchap_call_reads_from_calls_device): int8 calls of the units' distinct rows, their counts, rows per
    unit [U], the two offset arrays [U], n_alleles int8 [U, M].  Uploads them and enqueues the fill on torch's current stream (no
    synchronisation).  Returns (reads float64 [U, n_reads, M, max_allele], read_counts int64 [U, n_reads]) as torch tensors:
    encoding.encode_read_distributions of every unit's rows without qualities, padded to n_reads with NaN rows of count 0."""
    return _call_reads(calls, counts, unit_rows, unit_call_off, unit_count_off, n_alleles, n_reads, max_allele, error_rate, device)


def call_reads_from_calls_quals(calls, quals, counts, unit_rows, unit_call_off, unit_count_off, n_alleles, n_reads, max_allele,
                                error_rate=0.0024, n_qual=None, device=None):
    """call_reads_from_calls with base qualities in use (mchap_call_reads_from_calls_quals_device): quals int16, laid out like calls.
    The two probability tables -- p_call[q] = prob_of_qual(q) * (1 - error_rate) and p_other[q] = (1 - p_call[q]) / 3, formed as
    encoding.encode_read_distributions / as_probabilistic form them -- hold n_qual entries: by default one more than the largest
    quality of a called cell of the units.  Returns the same pair of torch tensors: encoding.encode_read_distributions of every
    unit's rows with their qualities, padded to n_reads with NaN rows of count 0."""
    return _call_reads(calls, counts, unit_rows, unit_call_off, unit_count_off, n_alleles, n_reads, max_allele, error_rate, device,
                       quals=quals, n_qual=n_qual)


def _call_reads(calls, counts, unit_rows, unit_call_off, unit_count_off, n_alleles, n_reads, max_allele, error_rate, device,
                quals=None, n_qual=None):
    """call_reads_from_calls, or with `quals` call_reads_from_calls_quals: the host-side checks, the upload and the fill."""
    from .blockpath import _ragged_arange, qual_prob_table

    name = "call_reads_from_calls" if quals is None else "call_reads_from_calls_quals"
    torch = _torch()
    dev = _device(torch, device)
    calls = np.ascontiguousarray(calls, dtype=np.int8).reshape(-1)
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    rows = np.ascontiguousarray(unit_rows, dtype=np.int64)
    c_off = np.ascontiguousarray(unit_call_off, dtype=np.int64)
    n_off = np.ascontiguousarray(unit_count_off, dtype=np.int64)
    nal = np.ascontiguousarray(n_alleles, dtype=np.int8)
    U, M = nal.shape
    R, A = int(n_reads), int(max_allele)
    host = [calls, counts, rows, c_off, n_off, nal.reshape(-1)]
    if quals is not None:
        quals = np.ascontiguousarray(quals, dtype=np.int16).reshape(-1)
        host.insert(1, quals)
    if not (rows.shape == c_off.shape == n_off.shape == (U,)) or R < 1 or M < 1 or A < 1 or (quals is not None and len(quals) != len(calls)):
        raise AssertionError("%s: per-unit arrays of one length, %sn_reads, positions and max_allele at least 1"
                             % (name, "" if quals is None else "as many qualities as calls, "))
    # (the kernel reads calls / quals / counts at these offsets: checked here, where the arrays are still on the host)
    if U and (rows.min() < 0 or rows.max() > R or c_off.min() < 0 or n_off.min() < 0 or (c_off + rows * M).max() > len(calls)
              or (n_off + rows).max() > len(counts)):
        raise AssertionError("%s: a unit's rows lie outside calls / counts, or exceed n_reads" % name)
    up = lambda a: torch.from_numpy(a).to(dev) if a.size else None  # noqa: E731
    # the probability of a called cell's allele and of each other allele, as encoding.encode_read_distributions / as_probabilistic
    # form them: two numbers, or with qualities two tables
    if quals is None:
        fill = _lib.lib().mchap_call_reads_from_calls_device
        p_call = 1.0 - error_rate
        d_tab, probs = [], (C.c_double(p_call), C.c_double((1.0 - p_call) / 3.0))
    else:
        fill = _lib.lib().mchap_call_reads_from_calls_quals_device
        # ... which the kernel reads at the qualities of the units' called cells
        owner, k = _ragged_arange(rows * M)
        used = c_off[owner] + k
        q_called = quals[used][calls[used] >= 0]
        n_qual = int(q_called.max(initial=0)) + 1 if n_qual is None else int(n_qual)
        if n_qual < 1 or (len(q_called) and (q_called.min() < 0 or q_called.max() >= n_qual)):
            raise AssertionError("%s: the quality of a called cell lies outside the table (0 <= q < %d)" % (name, n_qual))
        p_call = qual_prob_table(error_rate, n_qual)
        d_tab = [up(np.ascontiguousarray(p_call)), up(np.ascontiguousarray((1.0 - p_call) / 3.0))]
        probs = (_ptr(d_tab[0]), _ptr(d_tab[1]), n_qual)
    d_in = [up(a) for a in host]
    d_reads = torch.empty((U, R, M, A), dtype=torch.float64, device=dev)
    d_counts = torch.empty((U, R), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(fill(U, *[_ptr(t) for t in d_in], R, M, A, *probs, _ptr(d_reads), _ptr(d_counts), C.c_void_p(stream)))
    # (the inputs were allocated and are consumed on this stream: the allocator reuses them only for later work of the same stream)
    return d_reads, d_counts


class CompactCallReads:
    """The reads of a shape group of `mchap call` / `mchap call-exact` in the compact form of blockpath.call_unit_inputs, standing
    where the float64 [U, n_reads, M, max_allele] tensor does: `shape`, `len`, indexing and numpy conversion give that tensor
    (formed on the host by blockpath.expand_call_units when someone asks for it: a stand-in sampler of the tests, the host classes
    on downloaded traces), `counts` the [U, n_reads] counts in the same way, and on_device() both as device tensors formed there
    from the int8 calls (and, where the group comes with base qualities, `quals`: int16 laid out like the calls) -- what application._group_inputs hands to CallingMCMC.start_batch_summaries and, through _run_exact_groups, to ExactDeviceBatch."""

    ndim, dtype = 4, np.dtype(np.float64)

    def __init__(self, calls, counts, unit_rows, unit_call_off, unit_count_off, n_alleles, n_reads, max_allele, error_rate=0.0024,
                 quals=None):
        self.compact = (calls, counts, unit_rows, unit_call_off, unit_count_off, n_alleles)
        self.quals = quals
        self.n_reads, self.max_allele, self.error_rate = int(n_reads), int(max_allele), error_rate
        self.shape = (n_alleles.shape[0], self.n_reads, n_alleles.shape[1], self.max_allele)
        self.counts = _CompactCallCounts(self)
        self._host = None

    def on_device(self, device=None):
        """(reads, read_counts) device tensors, the fill enqueued on torch's current stream."""
        # (through the public names: the tests count the fills by wrapping them)
        if self.quals is not None:
            return call_reads_from_calls_quals(self.compact[0], self.quals, *self.compact[1:], self.n_reads, self.max_allele,
                                               error_rate=self.error_rate, device=device)
        return call_reads_from_calls(*self.compact, self.n_reads, self.max_allele, error_rate=self.error_rate, device=device)

    def on_host(self):
        if self._host is None:
            from .blockpath import expand_call_units

            self._host = expand_call_units(*self.compact, self.n_reads, self.max_allele, error_rate=self.error_rate, quals=self.quals)
        return self._host

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, i):
        return self.on_host()[0][i]

    def __array__(self, dtype=None, copy=None):
        a = self.on_host()[0]
        return a if dtype is None else a.astype(dtype, copy=False)


class _CompactCallCounts:
    """CompactCallReads.counts: the [U, n_reads] int64 counts, formed with the tensor."""

    ndim, dtype = 2, np.dtype(np.int64)

    def __init__(self, reads):
        self.reads = reads
        self.shape = reads.shape[:2]

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, i):
        return self.reads.on_host()[1][i]

    def __array__(self, dtype=None, copy=None):
        a = self.reads.on_host()[1]
        return a if dtype is None else a.astype(dtype, copy=False)


class ExactDeviceBatch:
    """A batch of exact-caller units that share a shape, resident on one GPU: inputs are uploaded once, every output of
    mchap_exact_call_batch_device stays in HBM until asked for.

    reads float64 [U, R, M, A]; haplotypes int8 [U, H, M] (or [H, M] for all units); read_counts int64 [U, R] or None;
    prior None | (inbreeding scalar or [U], frequencies None | [H] | [U, H])."""

    def __init__(self, reads, ploidy, haplotypes, read_counts=None, prior=None, device=None, cache_joint=True):
        torch = _torch()
        dev = _device(torch, device)
        reads = np.ascontiguousarray(reads, dtype=np.float64)
        d_reads = torch.from_numpy(reads.reshape(-1)).to(dev)
        d_counts = None if read_counts is None else torch.from_numpy(
            np.ascontiguousarray(read_counts, dtype=np.int64).reshape(-1)).to(dev)
        self._setup(d_reads, reads.shape, ploidy, haplotypes, d_counts, prior, dev, cache_joint)

    @classmethod
    def from_device_reads(cls, reads, ploidy, haplotypes, read_counts=None, prior=None, device=None, cache_joint=True):
        """The batch over read tensors that are on the device already (call_reads_from_calls): reads a float64 torch tensor
        [U, R, M, A], read_counts an int64 torch tensor [U, R] or None; the other arguments as the constructor's.  Nothing is
        copied: the batch keeps the tensors."""
        torch = _torch()
        assert reads.dtype == torch.float64 and reads.dim() == 4 and reads.is_contiguous()
        if read_counts is not None:
            assert read_counts.dtype == torch.int64 and tuple(read_counts.shape) == tuple(reads.shape[:2]) and read_counts.is_contiguous()
        self = cls.__new__(cls)
        self._setup(reads.reshape(-1), tuple(reads.shape), ploidy, haplotypes, None if read_counts is None else read_counts.reshape(-1),
                    prior, reads.device if device is None else device, cache_joint)
        return self

    def _setup(self, d_reads, shape, ploidy, haplotypes, d_counts, prior, dev, cache_joint):
        """Everything after the reads are on the device: haplotypes, prior, workspace."""
        torch = _torch()
        self.torch = torch
        self.device = dev
        U, R, M, A = (int(x) for x in shape)
        haps = np.asarray(haplotypes, dtype=np.int8)
        if haps.ndim == 2:
            haps = np.broadcast_to(haps, (U,) + haps.shape)
        haps = np.array(haps)
        H = haps.shape[1]
        self.shape = (U, R, M, A, H, int(ploidy))
        self.G = comb(H + int(ploidy) - 1, int(ploidy))
        self.d_reads = d_reads
        self.d_haps = torch.from_numpy(haps.reshape(-1)).to(dev)
        self.d_counts = d_counts
        self.has_prior = 0 if prior is None else 1
        self.d_F = self.d_fr = None
        if prior is not None:
            F = np.array(np.broadcast_to(np.asarray(prior[0], dtype=np.float64), (U,)))
            self.d_F = torch.from_numpy(F).to(dev)
            if prior[1] is not None:
                fr = np.array(np.broadcast_to(np.asarray(prior[1], dtype=np.float64), (U, H)))
                self.d_fr = torch.from_numpy(fr.reshape(-1)).to(dev)
        self.ws_bytes = int(_lib.lib().mchap_exact_workspace_bytes(U, H, int(ploidy)))
        free, _ = torch.cuda.mem_get_info()
        if self.ws_bytes < 0 or self.ws_bytes > free:
            # beyond what the exact caller enumerates here (the reference has no limit but time): the programs write such a record
            # with FILTER=LIMIT (application._run_exact_groups)
            raise NotImplementedError("mchap_hip: ploidy %d over %d haplotypes: %s genotypes are beyond this build's exact caller "
                                      "(2^62 indices; the workspace must fit the device)" % (int(ploidy), H, self.G))
        if cache_joint:
            # room for llk + log prior of every genotype between the two passes of the streaming form (8 bytes each)
            # (taken only when it fits comfortably: else the plain workspace, whose second pass forms the values again)
            big = int(_lib.lib().mchap_exact_workspace_bytes_cached(U, H, int(ploidy)))
            free, _ = torch.cuda.mem_get_info()
            if big <= min(16 << 30, free // 2):
                self.ws_bytes = big
        self.d_ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=dev)
        self.out = {}

    def _buf(self, name, n, dtype):
        t = self.out.get(name)
        if t is None:
            t = self.torch.empty(n, dtype=dtype, device=self.device)
            self.out[name] = t
        return t

    def run(self, streaming=True, arrays=False, llks64=False):
        """Enqueue the exact caller on torch's current stream: the streaming outputs (posterior_mode), and / or the
        array outputs (likelihoods, posteriors and their summaries)."""
        torch = self.torch
        U, R, M, A, H, K = self.shape
        f64, outputs = torch.float64, {}
        if streaming:
            outputs.update(mode_alleles=(U * K, torch.int64), mode_llk=(U, f64), mode_prob=(U, f64), support_prob=(U, f64),
                           freqs=(U * H, f64), occur=(U * H, f64))
        if arrays:
            outputs.update(llks=(U * self.G, torch.float32), posteriors=(U * self.G, f64), arr_mode_alleles=(U * K, torch.int64),
                           arr_mode_prob=(U, f64), arr_support_prob=(U, f64), arr_freqs=(U * H, f64), arr_counts=(U * H, f64),
                           arr_occur=(U * H, f64))
            if llks64:
                outputs["llks64"] = (U * self.G, f64)
        self._run_only(**outputs)

    def _run_only(self, **outputs):
        """mchap_exact_call_batch_device for the named outputs alone ({name: (elements, dtype)}), on torch's current stream."""
        U, R, M, A, H, K = self.shape
        o = _lib.ExactOut()
        for nm, (n, dtype) in outputs.items():
            setattr(o, nm, self._buf(nm, n, dtype).data_ptr())
        stream = self.torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mchap_exact_call_batch_device(
            U, _ptr(self.d_reads), R, M, A, _ptr(self.d_counts), _ptr(self.d_haps), H, K, self.has_prior,
            _ptr(self.d_F), _ptr(self.d_fr), C.byref(o), _ptr(self.d_ws), C.c_int64(self.ws_bytes), C.c_void_p(stream)))

    def run_llks64(self):
        """The unrounded float64 likelihoods [U * G] alone, left on the device (what the frequency estimate keeps resident)."""
        self._run_only(llks64=(self.shape[0] * self.G, self.torch.float64))
        return self.out["llks64"]

    def run_freqs(self, frequencies=None):
        """The mean posterior allele frequencies [U, H] alone (streaming form, both passes), under the prior frequencies
        [U, H] given here in place of the batch's: one iteration of the frequency estimate's recompute path."""
        U, R, M, A, H, K = self.shape
        if frequencies is not None:
            fr = self.torch.from_numpy(np.ascontiguousarray(frequencies, dtype=np.float64).reshape(-1))
            assert self.d_fr is not None and fr.numel() == U * H
            self.d_fr.copy_(fr)
        self._run_only(freqs=(U * H, self.torch.float64))
        return self._host("freqs", (U, H))

    def _host(self, name, shape):
        return self.out[name].cpu().numpy().reshape(shape)

    def mode_results(self):
        """(alleles [U, K], llk [U], prob [U], support_prob [U], freqs [U, H], occur [U, H]) of the streaming form."""
        U, R, M, A, H, K = self.shape
        return (self._host("mode_alleles", (U, K)), self._host("mode_llk", (U,)), self._host("mode_prob", (U,)),
                self._host("support_prob", (U,)), self._host("freqs", (U, H)), self._host("occur", (U, H)))

    def array_results(self, with_arrays=True):
        U, R, M, A, H, K = self.shape
        res = dict(alleles=self._host("arr_mode_alleles", (U, K)), prob=self._host("arr_mode_prob", (U,)),
                   support_prob=self._host("arr_support_prob", (U,)), freqs=self._host("arr_freqs", (U, H)),
                   counts=self._host("arr_counts", (U, H)), occur=self._host("arr_occur", (U, H)))
        if with_arrays:
            res["llks"] = self._host("llks", (U, self.G))
            res["posteriors"] = self._host("posteriors", (U, self.G))
        return res


class ExactFrequencyEstimate:
    """Prior allele frequencies by EM for a sub-block of whole records whose likelihoods are resident on the device
    (mchap_exact_em_counts_device, mchap_exact_em_update_device): the frequency rows, iteration counters and freeze flags of the
    records live on the device; an iteration is one counts launch per group added and one update launch.

    record_haps int [records]: haplotypes of each record; frequencies float64 [records, stride] (rows padded with 0): f_0;
    n_samples: samples of every record; ploidy_total: the sum of their ploidies."""

    def __init__(self, record_haps, frequencies, n_samples, ploidy_total, device=None):
        torch = _torch()
        self.torch = torch
        self.device = dev = _device(torch, device)
        fr = np.ascontiguousarray(frequencies, dtype=np.float64)
        self.n_records, self.stride = fr.shape
        self.n_samples, self.ploidy_total = int(n_samples), float(ploidy_total)
        haps = np.ascontiguousarray(record_haps, dtype=np.int32)
        assert haps.shape == (self.n_records,) and haps.min() >= 1 and haps.max() <= self.stride
        self.d_haps = torch.from_numpy(haps).to(dev)
        self.d_freqs = torch.from_numpy(fr.reshape(-1).copy()).to(dev)
        self.d_iters = torch.zeros(self.n_records, dtype=torch.int32, device=dev)
        self.d_active = torch.ones(self.n_records, dtype=torch.int32, device=dev)
        self.d_delta = torch.zeros(self.n_records, dtype=torch.float64, device=dev)
        self.d_slab = torch.zeros(self.n_records * self.n_samples * self.stride, dtype=torch.float64, device=dev)
        self.groups = []
        self.launches = 0   # iterations enqueued

    def add_group(self, llks64, n_haps, ploidy, inbreeding, unit_record, unit_sample):
        """The units of one shape (n_haps, ploidy): llks64 a float64 torch tensor [U * G] on the device (kept, not copied);
        inbreeding [U]; unit_record / unit_sample [U]: the record of the sub-block and the sample index of each unit."""
        torch, dev = self.torch, self.device
        rec = np.ascontiguousarray(unit_record, dtype=np.int32)
        smp = np.ascontiguousarray(unit_sample, dtype=np.int32)
        U = len(rec)
        G = comb(int(n_haps) + int(ploidy) - 1, int(ploidy))
        assert llks64.dtype == torch.float64 and llks64.numel() == U * G and llks64.is_contiguous()
        assert U == 0 or (rec.min() >= 0 and rec.max() < self.n_records and smp.min() >= 0 and smp.max() < self.n_samples)
        assert int(n_haps) <= self.stride
        wsb = int(_lib.lib().mchap_exact_em_workspace_bytes(U, int(n_haps), int(ploidy)))
        if wsb < 0:
            raise NotImplementedError("mchap_hip: ploidy %d over %d haplotypes: more than 2^62 genotypes" % (int(ploidy), int(n_haps)))
        self.groups.append(dict(
            U=U, H=int(n_haps), K=int(ploidy), llks=llks64, wsb=wsb,
            F=torch.from_numpy(np.array(np.broadcast_to(np.asarray(inbreeding, dtype=np.float64), (U,)))).to(dev),
            rec=torch.from_numpy(rec).to(dev), slot=torch.from_numpy(rec * np.int32(self.n_samples) + smp).to(dev),
            ws=torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)))

    def freeze(self, records):
        """Records that take no part (a group of theirs was refused): frozen from the start."""
        if len(records):
            self.d_active[self.torch.from_numpy(np.ascontiguousarray(records, dtype=np.int64)).to(self.device)] = 0

    def step(self, tolerance, max_iterations):
        """One iteration, enqueued on torch's current stream: the counts launches, then the update launch."""
        L = _lib.lib()
        stream = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        for g in self.groups:
            _lib.check(L.mchap_exact_em_counts_device(
                g["U"], _ptr(g["llks"]), g["H"], g["K"], _ptr(g["F"]), _ptr(g["rec"]), _ptr(g["slot"]), _ptr(self.d_freqs), self.stride,
                _ptr(self.d_active), _ptr(self.d_slab), _ptr(g["ws"]), C.c_int64(g["wsb"]), stream))
        _lib.check(L.mchap_exact_em_update_device(
            self.n_records, self.n_samples, _ptr(self.d_haps), self.stride, _ptr(self.d_slab), C.c_double(self.ploidy_total),
            C.c_double(float(tolerance)), int(max_iterations), _ptr(self.d_freqs), _ptr(self.d_iters), _ptr(self.d_active),
            _ptr(self.d_delta), stream))
        self.launches += 1

    def n_active(self):
        return int(self.d_active.sum().item())

    def run(self, max_iterations, tolerance, poll=4):
        """Iterations until every record is frozen: at most max_iterations launches, the number of active records read back every
        `poll` iterations only to stop launching early (a frozen record's units exit at once, so the result does not depend on it)."""
        if int(max_iterations) <= 0:
            return
        done = 0
        while done < int(max_iterations):
            self.step(tolerance, max_iterations)
            done += 1
            if done % max(1, int(poll)) == 0 and done < int(max_iterations) and self.n_active() == 0:
                break

    def results(self):
        """(frequencies [records, stride], iterations [records]) on the host."""
        return (self.d_freqs.cpu().numpy().reshape(self.n_records, self.stride), self.d_iters.cpu().numpy().astype(np.int64))


class ExactModelEvidence:
    """Model evidence of exact-caller units whose likelihoods are resident on the device (mchap_exact_evidence_device): for every
    unit and every candidate inbreeding F of its grid, log sum_g P(g | ploidy, F, f) P(reads | g) -- the normaliser of the unit's
    posterior under that prior.  The priors are normalised, so the values compare across F and across ploidies."""

    def __init__(self, device=None):
        self.torch = _torch()
        self.device = _device(self.torch, device)
        self.launches = 0   # groups enqueued

    def _tensor(self, a, dtype, np_dtype):
        if self.torch.is_tensor(a):
            assert a.dtype == dtype and a.is_contiguous()
            return a.to(self.device)
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(self.device)

    def add_group(self, llks64, n_haps, ploidy, inbreeding_grid, unit_row, freqs):
        """The units of one shape (n_haps, ploidy), enqueued on torch's current stream: llks64 a float64 torch tensor [U * G] on
        the device; inbreeding_grid [U, n_grid] (or [n_grid] for all units), every F in [0, 1) -- checked here, on the host copy --,
        or None: the flat genotype prior, one grid point, unit_row and freqs not used; unit_row [U]: each unit's row of freqs
        [rows, stride >= n_haps] (an array, or a float64 tensor on the device).  Returns the float64 tensor [U, n_grid] on the
        device."""
        torch, dev = self.torch, self.device
        H, K = int(n_haps), int(ploidy)
        if K < 1 or K > _lib.MAX_PLOIDY_GENERAL or comb(H + K - 1, K) >= 1 << 62:
            raise NotImplementedError("mchap_hip: ploidy %d over %d haplotypes is beyond this build's exact caller" % (K, H))
        G = comb(H + K - 1, K)
        assert llks64.dtype == torch.float64 and llks64.is_contiguous() and llks64.numel() % G == 0
        U = llks64.numel() // G
        d_F = d_row = d_fr = None
        n_grid, stride = 1, 0
        if inbreeding_grid is not None:
            F = np.asarray(inbreeding_grid, dtype=np.float64)
            if F.ndim == 1:
                F = np.broadcast_to(F, (U, F.shape[0]))
            if F.ndim != 2 or F.shape[0] != U or F.shape[1] < 1:
                raise ValueError("inbreeding_grid: [U, n_grid] with n_grid >= 1, got %r for %d units" % (F.shape, U))
            if not np.all((F >= 0.0) & (F < 1.0)):   # (False for NaN and infinities too)
                raise ValueError("inbreeding_grid: every F must lie in [0, 1)")
            n_grid = int(F.shape[1])
            d_F = torch.from_numpy(np.ascontiguousarray(F)).to(dev)
            d_row = self._tensor(unit_row, torch.int32, np.int32)
            d_fr = self._tensor(freqs, torch.float64, np.float64)
            assert d_row.numel() == U and d_fr.dim() == 2
            stride = int(d_fr.shape[1])
            if U and not torch.is_tensor(unit_row):
                rows = np.asarray(unit_row)
                assert int(rows.min()) >= 0 and int(rows.max()) < int(d_fr.shape[0])
        out = torch.empty((U, n_grid), dtype=torch.float64, device=dev)
        if U == 0:
            return out
        L = _lib.lib()
        wsb = int(L.mchap_exact_evidence_workspace_bytes(U, H, K, n_grid))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _lib.check(L.mchap_exact_evidence_device(
            U, _ptr(llks64), H, K, n_grid, _ptr(d_F), _ptr(d_row), _ptr(d_fr), stride, _ptr(out), _ptr(ws), C.c_int64(wsb),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return out


class ExactSnvPosteriors:
    """SNV genotype posteriors of exact-caller units whose likelihoods are resident on the device
    (mchap_exact_snv_posteriors_device): for every unit and SNV the unit's haplotype-genotype posterior summed over the SNV genotype
    each haplotype genotype implies there."""

    MAX_SNV_ALLELES = 4

    def __init__(self, device=None):
        self.torch = _torch()
        self.device = _device(self.torch, device)
        self.launches = 0   # groups enqueued
        self.log_norm = None   # the normalisers [U] of the last group, on the device

    _tensor = ExactModelEvidence._tensor

    def add_group(self, llks64, n_haps, ploidy, inbreeding, unit_row, freqs, hap_alleles):
        """The units of one shape (n_haps, ploidy), enqueued on torch's current stream: llks64 a float64 torch tensor [U * G] on
        the device; inbreeding [U] (or a scalar for all units), every F in [0, 1) -- checked here, on the host copy --, or None: the
        flat genotype prior, freqs not used; unit_row [U]: each unit's row of freqs [rows, stride >= n_haps] and of hap_alleles
        int8 [rows, n_haps, M], the SNV allele of every haplotype at every SNV (0 .. 3, checked here).  Returns the float64 tensor
        [U, M, S] on the device, S = C(A + ploidy - 1, ploidy) for A the largest number of SNV alleles in hap_alleles."""
        torch, dev = self.torch, self.device
        H, K = int(n_haps), int(ploidy)
        if K < 1 or K > _lib.MAX_PLOIDY_GENERAL or comb(H + K - 1, K) >= 1 << 62:
            raise NotImplementedError("mchap_hip: ploidy %d over %d haplotypes is beyond this build's exact caller" % (K, H))
        G = comb(H + K - 1, K)
        assert llks64.dtype == torch.float64 and llks64.is_contiguous() and llks64.numel() % G == 0
        U = llks64.numel() // G
        ha = np.ascontiguousarray(hap_alleles, dtype=np.int8)
        if ha.ndim != 3 or ha.shape[1] != H or ha.shape[2] < 1:
            raise ValueError("hap_alleles: [rows, %d, M] with M >= 1, got %r" % (H, ha.shape))
        if ha.size and (int(ha.min()) < 0 or int(ha.max()) >= self.MAX_SNV_ALLELES):
            raise ValueError("hap_alleles: every SNV allele must lie in 0..%d" % (self.MAX_SNV_ALLELES - 1))
        M, A = int(ha.shape[2]), int(ha.max()) + 1 if ha.size else 1
        S = comb(A + K - 1, K)
        rows = np.ascontiguousarray(unit_row, dtype=np.int32)
        assert rows.shape == (U,) and (U == 0 or (int(rows.min()) >= 0 and int(rows.max()) < ha.shape[0]))
        d_F = d_fr = None
        stride = 0
        if inbreeding is not None:
            F = np.array(np.broadcast_to(np.asarray(inbreeding, dtype=np.float64), (U,)))
            if not np.all((F >= 0.0) & (F < 1.0)):   # (False for NaN and infinities too)
                raise ValueError("inbreeding: every F must lie in [0, 1)")
            d_F = torch.from_numpy(F).to(dev)
            d_fr = self._tensor(freqs, torch.float64, np.float64)
            assert d_fr.dim() == 2 and (U == 0 or int(rows.max()) < int(d_fr.shape[0]))
            stride = int(d_fr.shape[1])
        out = torch.empty((U, M, S), dtype=torch.float64, device=dev)
        self.log_norm = torch.empty(U, dtype=torch.float64, device=dev)
        if U == 0:
            return out
        L = _lib.lib()
        wsb = int(L.mchap_exact_snv_workspace_bytes(U, H, K, M, A))
        free, _ = torch.cuda.mem_get_info()
        if wsb < 0 or wsb > free:
            raise NotImplementedError("mchap_hip: SNV posteriors of %d units of ploidy %d over %d haplotypes: the workspace does not "
                                      "fit the device" % (U, K, H))
        d_row = torch.from_numpy(rows).to(dev)
        d_ha = torch.from_numpy(ha.reshape(-1)).to(dev)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _lib.check(L.mchap_exact_snv_posteriors_device(
            U, _ptr(llks64), H, K, M, A, _ptr(d_F), _ptr(d_row), _ptr(d_fr), stride, _ptr(d_ha), _ptr(out), _ptr(self.log_norm),
            _ptr(ws), C.c_int64(wsb), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return out


class ExactReadSupport:
    """Expected read depth of every haplotype for exact-caller units whose reads and likelihoods are resident on the device
    (mchap_exact_allele_support_device): the responsibility of every haplotype for every read under every genotype, averaged over
    the unit's genotype posterior and summed over the reads with their weights."""

    def __init__(self, device=None):
        self.torch = _torch()
        self.device = _device(self.torch, device)
        self.launches = 0      # groups enqueued
        self.log_norm = None   # the normalisers [U] of the last group, on the device

    _tensor = ExactModelEvidence._tensor

    def add_group(self, batch, llks64, inbreeding, unit_row, freqs, per_read=False):
        """The units of an ExactDeviceBatch -- its reads, haplotypes and read counts are on the device already --, enqueued on
        torch's current stream: llks64 the batch's float64 likelihoods [U * G] (run_llks64); inbreeding [U] (or a scalar for all
        units), every F in [0, 1) -- checked here, on the host copy --, or None: the flat genotype prior, unit_row and freqs not
        used; unit_row [U]: each unit's row of freqs [rows, stride >= n_haps].  Returns the float64 tensor depth [U, H] on the
        device -- with per_read=True the pair (depth, read_post [U, R, H]).  A shape the library refuses (ploidy, genotype count,
        tables beyond the LDS, a workspace beyond the device): NotImplementedError."""
        torch, dev = self.torch, self.device
        U, R, M, A, H, K = batch.shape
        if K < 1 or K > _lib.MAX_PLOIDY_GENERAL or comb(H + K - 1, K) >= 1 << 62:
            raise NotImplementedError("mchap_hip: ploidy %d over %d haplotypes is beyond this build's exact caller" % (K, H))
        assert llks64.dtype == torch.float64 and llks64.is_contiguous() and llks64.numel() == U * batch.G
        L = _lib.lib()
        if U and int(L.mchap_exact_support_tile(R, H, K)) == 0:
            raise NotImplementedError("mchap_hip: allele support over %d haplotypes: not even 64 read rows of its tables fit the LDS" % H)
        d_F = d_fr = d_row = None
        stride = 0
        if inbreeding is not None:
            F = np.array(np.broadcast_to(np.asarray(inbreeding, dtype=np.float64), (U,)))
            if not np.all((F >= 0.0) & (F < 1.0)):   # (False for NaN and infinities too)
                raise ValueError("inbreeding: every F must lie in [0, 1)")
            rows = np.ascontiguousarray(unit_row, dtype=np.int32)
            d_fr = self._tensor(freqs, torch.float64, np.float64)
            assert d_fr.dim() == 2 and int(d_fr.shape[1]) >= H
            assert rows.shape == (U,) and (U == 0 or (int(rows.min()) >= 0 and int(rows.max()) < int(d_fr.shape[0])))
            stride = int(d_fr.shape[1])
            d_F = torch.from_numpy(F).to(dev)
            d_row = torch.from_numpy(rows).to(dev)
        depth = torch.empty((U, H), dtype=torch.float64, device=dev)
        self.log_norm = torch.empty(U, dtype=torch.float64, device=dev)
        if U == 0:
            return (depth, torch.empty((0, R, H), dtype=torch.float64, device=dev)) if per_read else depth
        wsb = int(L.mchap_exact_support_workspace_bytes(U, R, H, K, 1 if per_read else 0))
        free, _ = torch.cuda.mem_get_info()
        if wsb < 0 or wsb + (U * R * H * 8 if per_read else 0) > free:
            raise NotImplementedError("mchap_hip: allele support of %d units of ploidy %d over %d haplotypes: the workspace does not "
                                      "fit the device" % (U, K, H))
        post = torch.empty((U, R, H), dtype=torch.float64, device=dev) if per_read else None
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _lib.check(L.mchap_exact_allele_support_device(
            U, _ptr(batch.d_reads), R, M, A, _ptr(batch.d_counts), _ptr(batch.d_haps), H, K, _ptr(llks64), _ptr(d_F), _ptr(d_row),
            _ptr(d_fr), stride, _ptr(depth), _ptr(post), _ptr(self.log_norm), _ptr(ws), C.c_int64(wsb),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return (depth, post) if per_read else depth


class ExactCross:
    """Progeny calls under their parents' cross prior for exact-caller units whose likelihoods are resident on the device
    (mchap_exact_gametes_device, mchap_exact_cross_prior_device, mchap_exact_cross_posterior_device): the parents' gamete tables, the
    cross prior of a record, the progeny's posterior under it.  `tables` keeps what the caller puts there -- the gamete rows of a
    block's records between the parents' groups and the progeny's -- on the device."""

    def __init__(self, device=None):
        self.torch = _torch()
        self.device = _device(self.torch, device)
        self.launches = 0      # calls enqueued
        self.log_norm = None   # the parents' normalisers [U] of the last gametes call, on the device
        self.tables = {}

    _tensor = ExactModelEvidence._tensor

    @staticmethod
    def _shape(H, K):
        if K < 1 or K > _lib.MAX_PLOIDY_GENERAL or comb(H + K - 1, K) >= 1 << 62:
            raise NotImplementedError("mchap_hip: ploidy %d over %d haplotypes is beyond this build's exact caller" % (K, H))
        return comb(H + K - 1, K)

    def _prior(self, U, H, inbreeding, unit_row, freqs):
        """(d_F or None, d_row, d_fr, stride) of a group: F checked on the host copy, the rows against the table."""
        torch, dev = self.torch, self.device
        d_F = None
        if inbreeding is not None:
            F = np.array(np.broadcast_to(np.asarray(inbreeding, dtype=np.float64), (U,)))
            if not np.all((F >= 0.0) & (F < 1.0)):   # (False for NaN and infinities too)
                raise ValueError("inbreeding: every F must lie in [0, 1)")
            d_F = torch.from_numpy(F).to(dev)
        rows = np.ascontiguousarray(unit_row, dtype=np.int32)
        d_fr = self._tensor(freqs, torch.float64, np.float64)
        assert d_fr.dim() == 2 and int(d_fr.shape[1]) >= H
        assert rows.shape == (U,) and (U == 0 or (int(rows.min()) >= 0 and int(rows.max()) < int(d_fr.shape[0])))
        return d_F, torch.from_numpy(rows).to(dev), d_fr, int(d_fr.shape[1])

    def _workspace(self, wsb, extra, what):
        free, _ = self.torch.cuda.mem_get_info()
        if wsb < 0 or wsb + extra > free:
            raise NotImplementedError("mchap_hip: %s: the shape is refused, or its workspace does not fit the device" % what)
        return self.torch.empty(max(wsb, 16), dtype=self.torch.uint8, device=self.device)

    def gametes(self, llks64, n_haps, ploidy, inbreeding, unit_row, freqs, gamete_error):
        """The gamete tables of parent units of one shape (n_haps, even ploidy), enqueued on torch's current stream: llks64 a
        float64 tensor [U * G] on the device; inbreeding [U] (or a scalar), every F in [0, 1), or None: the flat genotype prior;
        unit_row [U]: each unit's row of freqs [rows, stride >= n_haps] -- read under the flat prior too, for the gamete error's
        multinomial --; gamete_error [U] (or a scalar), every e in [0, 1].  F and e are checked here, on the host copies.  Returns
        the float64 tensor [U, C(H + t - 1, t)] on the device, NaN rows for a unit without a finite genotype.  A shape the library
        refuses: NotImplementedError."""
        torch, dev = self.torch, self.device
        H, K = int(n_haps), int(ploidy)
        G = self._shape(H, K)
        if K % 2:
            raise ValueError("gametes: a parent of odd ploidy %d" % K)
        assert llks64.dtype == torch.float64 and llks64.is_contiguous() and llks64.numel() % G == 0
        U = llks64.numel() // G
        e = np.array(np.broadcast_to(np.asarray(gamete_error, dtype=np.float64), (U,)))
        if not np.all((e >= 0.0) & (e <= 1.0)):
            raise ValueError("gamete_error: every e must lie in [0, 1]")
        d_F, d_row, d_fr, stride = self._prior(U, H, inbreeding, unit_row, freqs)
        NA = comb(H + K // 2 - 1, K // 2)
        out = torch.empty((U, NA), dtype=torch.float64, device=dev)
        self.log_norm = torch.empty(U, dtype=torch.float64, device=dev)
        if U == 0:
            return out
        L = _lib.lib()
        wsb = int(L.mchap_exact_gametes_workspace_bytes(U, H, K))
        ws = self._workspace(wsb, 0, "gametes of %d units of ploidy %d over %d haplotypes" % (U, K, H))
        d_e = torch.from_numpy(e).to(dev)
        _lib.check(L.mchap_exact_gametes_device(
            U, _ptr(llks64), H, K, _ptr(d_F), _ptr(d_row), _ptr(d_fr), stride, _ptr(d_e), _ptr(out), _ptr(self.log_norm), _ptr(ws),
            C.c_int64(wsb), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return out

    def cross_prior(self, gametes_p, gametes_q, n_haps, ploidy_p, ploidy_q):
        """log X [rows, G_c] on the device from the two parents' gamete tables [rows, .] (float64 tensors on the device, a row per
        record): exactly -inf where every product is 0."""
        torch, dev = self.torch, self.device
        H, KP, KQ = int(n_haps), int(ploidy_p), int(ploidy_q)
        if KP < 2 or KQ < 2 or KP % 2 or KQ % 2:
            raise ValueError("cross_prior: parents of even ploidy are needed, got %d and %d" % (KP, KQ))
        self._shape(H, KP), self._shape(H, KQ)
        GC = self._shape(H, KP // 2 + KQ // 2)
        rows = int(gametes_p.shape[0])
        for t, K in ((gametes_p, KP), (gametes_q, KQ)):
            assert t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (rows, comb(H + K // 2 - 1, K // 2))
        free, _ = torch.cuda.mem_get_info()
        if rows * GC * 8 > free:
            raise NotImplementedError("mchap_hip: the cross prior of %d records over %d genotypes does not fit the device" % (rows, GC))
        out = torch.empty((rows, GC), dtype=torch.float64, device=dev)
        if rows:
            _lib.check(_lib.lib().mchap_exact_cross_prior_device(rows, _ptr(gametes_p), _ptr(gametes_q), H, KP, KQ, _ptr(out),
                                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            self.launches += 1
        return out

    def posteriors(self, llks64, n_haps, ploidy, log_cross, unit_row, inbreeding=None, freqs=None, full=False):
        """The progeny units of one shape under the cross prior: llks64 [U * G_c] and log_cross [rows, G_c] float64 tensors on the
        device, unit_row [U] each unit's row of log_cross -- and of freqs [rows, stride >= n_haps], the calling prior's
        frequencies (inbreeding [U], a scalar, or None: the flat genotype prior).  Returns float64 / int64 tensors on the device:
        (log_z [U], mode [U], mode_prob [U], log_norm [U]) -- the cross evidence, the first maximum in VCF order (-1: none), its
        probability, the unit's evidence under its calling prior -- and with full=True a fifth, the posterior [U, G_c]."""
        torch, dev = self.torch, self.device
        H, K = int(n_haps), int(ploidy)
        G = self._shape(H, K)
        assert llks64.dtype == torch.float64 and llks64.is_contiguous() and llks64.numel() % G == 0
        assert log_cross.dtype == torch.float64 and log_cross.is_contiguous() and log_cross.dim() == 2 and int(log_cross.shape[1]) == G
        U = llks64.numel() // G
        rows = np.ascontiguousarray(unit_row, dtype=np.int32)
        assert rows.shape == (U,) and (U == 0 or (int(rows.min()) >= 0 and int(rows.max()) < int(log_cross.shape[0])))
        d_F = d_fr = None
        stride = 0
        d_row = torch.from_numpy(rows).to(dev)
        if inbreeding is not None:
            d_F, _, d_fr, stride = self._prior(U, H, inbreeding, unit_row, freqs)
        log_z, prob, norm = (torch.empty(U, dtype=torch.float64, device=dev) for _ in range(3))
        mode = torch.empty(U, dtype=torch.int64, device=dev)
        post = None
        if U:
            L = _lib.lib()
            wsb = int(L.mchap_exact_cross_posterior_workspace_bytes(U, H, K))
            ws = self._workspace(wsb, U * G * 8 if full else 0, "cross posterior of %d units of ploidy %d over %d haplotypes" % (U, K, H))
            post = torch.empty((U, G), dtype=torch.float64, device=dev) if full else None
            _lib.check(L.mchap_exact_cross_posterior_device(
                U, _ptr(llks64), H, K, _ptr(log_cross), _ptr(d_row), _ptr(d_F), _ptr(d_row), _ptr(d_fr), stride, _ptr(log_z),
                _ptr(mode), _ptr(prob), _ptr(norm), _ptr(post), _ptr(ws), C.c_int64(wsb),
                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            self.launches += 1
        elif full:
            post = torch.empty((0, G), dtype=torch.float64, device=dev)
        return (log_z, mode, prob, norm, post) if full else (log_z, mode, prob, norm)


class ExactParentage:
    """Candidate parent pairs per progeny for exact-caller units whose likelihoods are resident on the device
    (mchap_exact_parentage_device): the cross evidence of every progeny of a record under every pair of rows of two gamete tables.
    The rows are what ExactCross.gametes returns for the candidates (`gametes` here: one gamete error for all), and the
    population's row of the unknown parent (`population`).  The definition: application.parentage_unit."""

    TMAX = 7   # the largest gamete size (exact_parentage_kernel.hpp PARENTAGE_TMAX)

    def __init__(self, device=None):
        self.torch = _torch()
        self.device = _device(self.torch, device)
        self.cross = ExactCross(self.device)
        self.launches = 0      # calls enqueued (the gamete launches are counted in self.cross)

    _tensor = ExactModelEvidence._tensor

    @classmethod
    def _gametes(cls, H, t):
        if t < 1 or t > cls.TMAX or comb(H + t - 1, t) >= 1 << 62:
            raise NotImplementedError("mchap_hip: gametes of %d haplotypes over %d are beyond this build's parentage kernel" % (t, H))
        return comb(H + t - 1, t)

    def gametes(self, llks64, n_haps, ploidy, inbreeding, unit_row, freqs, gamete_error):
        """The candidates' gamete rows [U, C(H + t - 1, t)]: ExactCross.gametes at one gamete error in [0, 1] for every unit -- checked
        there, on the host copy."""
        return self.cross.gametes(llks64, n_haps, ploidy, inbreeding, unit_row, freqs, float(gamete_error))

    def population(self, freqs, n_haps, t, out=None):
        """Mult(a; t, f) of every gamete of t haplotypes for the records' frequencies freqs [R, stride >= n_haps] -- the unknown
        parent's row, what the gamete launch returns at a gamete error of 1 --, formed on the device: a float64 tensor [R, NA], or
        written into out [R, NA], a view whose rows may be strided (a row of a table)."""
        torch = self.torch
        H, t = int(n_haps), int(t)
        NA = self._gametes(H, t)
        d_fr = self._tensor(freqs, torch.float64, np.float64)
        assert d_fr.dim() == 2 and int(d_fr.shape[1]) >= H
        R = int(d_fr.shape[0])
        if out is None:
            out = torch.empty((R, NA), dtype=torch.float64, device=self.device)
        assert out.dtype == torch.float64 and tuple(out.shape) == (R, NA) and (R == 0 or (out.stride(1) == 1 and out.stride(0) >= NA))
        if R:
            _lib.check(_lib.lib().mchap_exact_parentage_population_device(
                R, _ptr(d_fr), int(d_fr.shape[1]), H, t, _ptr(out), C.c_int64(int(out.stride(0)) if R > 1 else NA),
                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            self.launches += 1
        return out

    def table(self, rows, freqs, n_haps, t):
        """The table [R, n + 1, NA] of a gamete size: rows [R, n, NA] the candidates' gamete rows (a float64 tensor on the device,
        n may be 0, or None), and the population's row of every record last."""
        torch = self.torch
        H, t = int(n_haps), int(t)
        NA = self._gametes(H, t)
        d_fr = self._tensor(freqs, torch.float64, np.float64)
        R = int(d_fr.shape[0])
        n = 0 if rows is None else int(rows.shape[1])
        out = torch.empty((R, n + 1, NA), dtype=torch.float64, device=self.device)
        if n:
            assert rows.dtype == torch.float64 and tuple(rows.shape) == (R, n, NA)
            out[:, :n] = rows
        self.population(d_fr, H, t, out[:, n])
        return out

    @staticmethod
    def workspace_bytes(n_records, n_progeny, n_a, n_b, n_haps, t_a, t_b):
        """The bytes of workspace a call needs, or -1 for a shape the kernels refuse."""
        return int(_lib.lib().mchap_exact_parentage_workspace_bytes(int(n_records), int(n_progeny), int(n_a), int(n_b), int(n_haps),
                                                                    int(t_a), int(t_b)))

    def log_evidence(self, gametes_a, gametes_b, llks_c, n_haps, t_a, t_b, progeny_reads=None, workspace_limit=None):
        """The records of one shape, enqueued on torch's current stream: gametes_a [R, n_a, NA], gametes_b [R, n_b, NB] float64
        tensors on the device (they may be one tensor), llks_c [R * C * G_c] the progeny's likelihoods, progeny_reads [R, C] of
        0 / 1 (None: every progeny has reads).  workspace_limit: the bytes the caller offers (None: what the device has free); a
        workspace beyond it, or a shape the library refuses: NotImplementedError.  Returns log_z [R, C, n_a, n_b] on the device."""
        torch, dev = self.torch, self.device
        H, ta, tb = int(n_haps), int(t_a), int(t_b)
        NA, NB = self._gametes(H, ta), self._gametes(H, tb)
        GC = ExactCross._shape(H, ta + tb)
        for g, N in ((gametes_a, NA), (gametes_b, NB)):
            assert g.dtype == torch.float64 and g.is_contiguous() and g.dim() == 3 and int(g.shape[2]) == N and int(g.shape[1]) >= 1
        R, n_a, n_b = int(gametes_a.shape[0]), int(gametes_a.shape[1]), int(gametes_b.shape[1])
        assert int(gametes_b.shape[0]) == R
        assert llks_c.dtype == torch.float64 and llks_c.is_contiguous() and (R == 0 or llks_c.numel() % (R * GC) == 0)
        n = llks_c.numel() // (R * GC) if R else 0
        d_reads = None
        if progeny_reads is not None:
            reads = np.ascontiguousarray(progeny_reads, dtype=np.int32)
            assert reads.shape == (R, n)
            d_reads = torch.from_numpy(reads).to(dev)
        out = torch.empty((R, n, n_a, n_b), dtype=torch.float64, device=dev)
        if R == 0 or n == 0:
            return out
        wsb = self.workspace_bytes(R, n, n_a, n_b, H, ta, tb)
        limit = workspace_limit
        if limit is None:
            limit, _ = torch.cuda.mem_get_info()
        if wsb < 0 or wsb > limit:
            raise NotImplementedError("mchap_hip: parentage of %d records x %d progeny x %d columns over %d haplotypes: the shape is "
                                      "refused, or its workspace does not fit the device" % (R, n, n_b, H))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().mchap_exact_parentage_device(
            R, n, n_a, n_b, _ptr(gametes_a), _ptr(gametes_b), _ptr(llks_c), _ptr(d_reads), H, ta, tb, _ptr(out), _ptr(ws),
            C.c_int64(wsb), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return out


class ExactSelfing:
    """Selfed parents per progeny for exact-caller units whose likelihoods are resident on the device
    (mchap_exact_selfing_prior_device, mchap_exact_selfing_evidence_device): the genotype prior of a progeny whose two gametes are
    two meioses of one genotype drawn from a candidate's posterior, and the evidence of every progeny of a record under every
    candidate's such prior.  The definitions: application.selfing_prior, application.selfing_evidence."""

    def __init__(self, device=None):
        self.torch = _torch()
        self.device = _device(self.torch, device)
        self.launches = 0      # calls enqueued

    _tensor = ExactModelEvidence._tensor
    _prior = ExactCross._prior

    @staticmethod
    def prior_workspace_bytes(n_units, n_haps, ploidy):
        """The bytes of workspace a selfing_prior call needs, or -1 for a shape the kernels refuse."""
        return int(_lib.lib().mchap_exact_selfing_prior_workspace_bytes(int(n_units), int(n_haps), int(ploidy)))

    @staticmethod
    def evidence_workspace_bytes(n_records, n_progeny, n_candidates, n_haps, ploidy):
        """The bytes of workspace a log_evidence call needs, or -1 for a shape the kernels refuse."""
        return int(_lib.lib().mchap_exact_selfing_evidence_workspace_bytes(int(n_records), int(n_progeny), int(n_candidates),
                                                                           int(n_haps), int(ploidy)))

    def selfing_prior(self, llks64, n_haps, ploidy, inbreeding, unit_row, freqs, gamete_error, workspace_limit=None):
        """The selfing priors of candidate units of one shape (n_haps, even ploidy), enqueued on torch's current stream; the
        arguments are ExactCross.gametes': llks64 a float64 tensor [U * G] on the device; inbreeding [U] (or a scalar), every F in
        [0, 1), or None: the flat genotype prior; unit_row [U]: each unit's row of freqs [rows, stride >= n_haps]; gamete_error [U]
        (or a scalar), every e in [0, 1].  F and e are checked here, on the host copies.  Returns float64 tensors on the device:
        (log_self [U, G], self_prior [U, G], log_norm [U]) -- log S, S and the unit's normaliser --, NaN rows for a unit without a
        finite genotype.  A shape the library refuses, or a workspace beyond workspace_limit bytes (None: what the device has
        free): NotImplementedError."""
        torch, dev = self.torch, self.device
        H, K = int(n_haps), int(ploidy)
        G = ExactCross._shape(H, K)
        if K % 2:
            raise ValueError("selfing_prior: a parent of odd ploidy %d" % K)
        assert llks64.dtype == torch.float64 and llks64.is_contiguous() and llks64.numel() % G == 0
        U = llks64.numel() // G
        e = np.array(np.broadcast_to(np.asarray(gamete_error, dtype=np.float64), (U,)))
        if not np.all((e >= 0.0) & (e <= 1.0)):
            raise ValueError("gamete_error: every e must lie in [0, 1]")
        d_F, d_row, d_fr, stride = self._prior(U, H, inbreeding, unit_row, freqs)
        log_self, lin = (torch.empty((U, G), dtype=torch.float64, device=dev) for _ in range(2))
        norm = torch.empty(U, dtype=torch.float64, device=dev)
        if U == 0:
            return log_self, lin, norm
        wsb = self.prior_workspace_bytes(U, H, K)
        limit = workspace_limit
        if limit is None:
            limit, _ = torch.cuda.mem_get_info()
        if wsb < 0 or wsb > limit:
            raise NotImplementedError("mchap_hip: selfing prior of %d units of ploidy %d over %d haplotypes: the shape is refused, "
                                      "or its workspace does not fit the device" % (U, K, H))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        d_e = torch.from_numpy(e).to(dev)
        _lib.check(_lib.lib().mchap_exact_selfing_prior_device(
            U, _ptr(llks64), H, K, _ptr(d_F), _ptr(d_row), _ptr(d_fr), stride, _ptr(d_e), _ptr(log_self), _ptr(lin), _ptr(norm),
            _ptr(ws), C.c_int64(wsb), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return log_self, lin, norm

    def log_evidence(self, self_prior, llks_c, n_haps, ploidy, progeny_reads=None, workspace_limit=None):
        """The records of one shape, enqueued on torch's current stream: self_prior [R, n, G] the candidates' selfing priors (S, a
        float64 tensor on the device), llks_c [R * C * G] the progeny's likelihoods, progeny_reads [R, C] of 0 / 1 (None: every
        progeny has reads).  workspace_limit: the bytes the caller offers (None: what the device has free); a workspace beyond
        it, or a shape the library refuses: NotImplementedError.  Returns log_z [R, C, n] on the device."""
        torch, dev = self.torch, self.device
        H, K = int(n_haps), int(ploidy)
        G = ExactCross._shape(H, K)
        assert self_prior.dtype == torch.float64 and self_prior.is_contiguous() and self_prior.dim() == 3
        R, n = int(self_prior.shape[0]), int(self_prior.shape[1])
        assert int(self_prior.shape[2]) == G and n >= 1
        assert llks_c.dtype == torch.float64 and llks_c.is_contiguous() and (R == 0 or llks_c.numel() % (R * G) == 0)
        Cn = llks_c.numel() // (R * G) if R else 0
        d_reads = None
        if progeny_reads is not None:
            reads = np.ascontiguousarray(progeny_reads, dtype=np.int32)
            assert reads.shape == (R, Cn)
            d_reads = torch.from_numpy(reads).to(dev)
        out = torch.empty((R, Cn, n), dtype=torch.float64, device=dev)
        if R == 0 or Cn == 0:
            return out
        wsb = self.evidence_workspace_bytes(R, Cn, n, H, K)
        limit = workspace_limit
        if limit is None:
            limit, _ = torch.cuda.mem_get_info()
        if wsb < 0 or wsb > limit:
            raise NotImplementedError("mchap_hip: selfing evidence of %d records x %d progeny x %d candidates over %d haplotypes: the "
                                      "shape is refused, or its workspace does not fit the device" % (R, Cn, n, H))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().mchap_exact_selfing_evidence_device(
            R, Cn, n, _ptr(self_prior), _ptr(llks_c), _ptr(d_reads), H, K, _ptr(out), _ptr(ws), C.c_int64(wsb),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return out


class ExactIdentity:
    """Sample pairs by shared-genotype evidence for exact-caller units whose likelihoods are resident on the device
    (mchap_exact_identity_device): per record the log Bayes factor of "one genotype read twice" against two independent draws
    from the calling prior, for every pair of the record's samples -- one ploidy, one prior.  The definition:
    application.identity_unit."""

    def __init__(self, device=None):
        self.torch = _torch()
        self.device = _device(self.torch, device)
        self.launches = 0      # calls enqueued

    _tensor = ExactModelEvidence._tensor

    @staticmethod
    def workspace_bytes(n_records, n_samples, n_haps, ploidy):
        """The bytes of workspace a call needs, or -1 for a shape the kernels refuse."""
        return int(_lib.lib().mchap_exact_identity_workspace_bytes(int(n_records), int(n_samples), int(n_haps), int(ploidy)))

    def log_bayes_factors(self, llks, n_haps, ploidy, inbreeding, rows, frequencies, log_norm, error, reads=None, workspace_limit=None, phases=3, workspace=None):
        """The records of one shape, enqueued on torch's current stream: llks [R * n * G] a float64 tensor on the device, the n
        samples of a record side by side; inbreeding: the one F in [0, 1) of every sample, or None for the flat prior (rows and
        frequencies are then not used); rows [R]: each record's row of frequencies [rows, stride >= n_haps] (an array, or a
        float64 tensor on the device); log_norm [R, n]: every sample's evidence under that prior (ExactModelEvidence.add_group, one
        grid point), a float64 tensor on the device; error in [0, 1]; reads [R, n] of read weights, 0: no reads (None: every
        sample has reads).  workspace_limit: the bytes the caller offers (None: what the device has free); a workspace beyond it,
        or a shape the library refuses: NotImplementedError.  phases, workspace: for tools/identity_once.py, which times the launches
        that form the rows a (phases = 1) and the product (phases = 2) apart over one uint8 workspace tensor of workspace_bytes.
        Returns lbf [R, n, n] on the device, the diagonal NaN."""
        torch, dev = self.torch, self.device
        H, K, e = int(n_haps), int(ploidy), float(error)
        if not 0.0 <= e <= 1.0:   # (False for NaN too)
            raise ValueError("identity: the error lies in [0, 1]")
        if K < 1 or K > _lib.MAX_PLOIDY_GENERAL or comb(H + K - 1, K) >= 1 << 62:
            raise NotImplementedError("mchap_hip: ploidy %d over %d haplotypes is beyond this build's exact caller" % (K, H))
        G = comb(H + K - 1, K)
        assert log_norm.dtype == torch.float64 and log_norm.is_contiguous() and log_norm.dim() == 2
        R, n = int(log_norm.shape[0]), int(log_norm.shape[1])
        assert llks.dtype == torch.float64 and llks.is_contiguous() and llks.numel() == R * n * G
        d_fr, stride, F = None, 0, None
        if inbreeding is not None:
            F = C.c_double(float(inbreeding))
            if not 0.0 <= F.value < 1.0:
                raise ValueError("identity: F must lie in [0, 1)")
            table = self._tensor(frequencies, torch.float64, np.float64)
            at = np.asarray(rows, dtype=np.int64)
            assert table.dim() == 2 and int(table.shape[1]) >= H and at.shape == (R,)
            assert R == 0 or (int(at.min()) >= 0 and int(at.max()) < int(table.shape[0]))
            d_fr = table[torch.from_numpy(at).to(dev)].contiguous()
            stride = int(d_fr.shape[1])
        d_reads = None
        if reads is not None:
            w = np.ascontiguousarray(np.asarray(reads) != 0, dtype=np.int32)
            assert w.shape == (R, n)
            d_reads = torch.from_numpy(w).to(dev)
        out = torch.empty((R, n, n), dtype=torch.float64, device=dev)
        if R == 0 or n == 0:
            return out
        wsb = self.workspace_bytes(R, n, H, K)
        limit = workspace_limit
        if limit is None:
            limit, _ = torch.cuda.mem_get_info()
        if wsb < 0 or wsb > limit:
            raise NotImplementedError("mchap_hip: identity of %d records x %d samples of ploidy %d over %d haplotypes: the shape is "
                                      "refused, or its workspace does not fit the device" % (R, n, K, H))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev) if workspace is None else workspace
        assert ws.numel() >= wsb
        _lib.check(_lib.lib().mchap_exact_identity_device(
            R, n, _ptr(llks), H, K, None if F is None else C.addressof(F), _ptr(d_fr), stride, _ptr(log_norm), C.c_double(e),
            _ptr(d_reads), _ptr(out), int(phases), _ptr(ws), C.c_int64(wsb), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return out


class ExactFamily:
    """The parents and the progeny of one cross called jointly for exact-caller units whose likelihoods are resident on the device
    (mchap_exact_family_device): per record the exact joint posterior of the two parents and all progeny, its marginals and every
    progeny's predictive log evidence.  The definition: application.family_unit."""

    def __init__(self, device=None):
        self.torch = _torch()
        self.device = _device(self.torch, device)
        self.launches = 0      # calls enqueued

    _tensor = ExactModelEvidence._tensor
    _shape = staticmethod(ExactCross._shape)

    @staticmethod
    def workspace_bytes(n_records, n_haps, ploidy_p, ploidy_q, force_fallback=False):
        """The bytes of workspace a call over n_records records needs (the [G_P][G_Q] array of every record and the smaller
        stages), or -1 for a shape the kernels refuse."""
        return int(_lib.lib().mchap_exact_family_workspace_bytes(int(n_records), int(n_haps), int(ploidy_p), int(ploidy_q),
                                                                 1 if force_fallback else 0))

    def call(self, llks_p, llks_q, llks_c, n_haps, ploidy_p, ploidy_q, freqs, gamete_error=(0.01, 0.01), inbreeding_p=None,
             inbreeding_q=None, progeny_reads=None, full=False, force_fallback=False, workspace_limit=None):
        """The records of one shape, enqueued on torch's current stream.  llks_p [R * G_P], llks_q [R * G_Q], llks_c
        [R * n * G_c] float64 tensors on the device (llks_c None or empty: no progeny); freqs [R, stride >= n_haps] the records'
        calling frequencies; gamete_error (e_P, e_Q), each a scalar or [R], every e in [0, 1]; inbreeding_p / _q [R] (or a
        scalar), every F in [0, 1), or None: the flat genotype prior; progeny_reads [R, n] of 0 / 1 (None: every progeny has
        reads).  F and e are checked here, on the host copies.  workspace_limit: the bytes the caller offers (None: what the device
        has free); a workspace beyond it, or a shape the library refuses: NotImplementedError.  Returns a dict of tensors on the
        device: post_p [R, G_P], post_q [R, G_Q], mode_p, mode_q [R] int64 (-1: a null record), prob_p, prob_q [R], log_z [R],
        mode_c [R, n] int64, prob_c [R, n], pred [R, n], and with full=True q [R, n, G_c]."""
        torch, dev = self.torch, self.device
        H, KP, KQ = int(n_haps), int(ploidy_p), int(ploidy_q)
        if KP < 2 or KQ < 2 or KP % 2 or KQ % 2:
            raise ValueError("family: parents of even ploidy are needed, got %d and %d" % (KP, KQ))
        GP, GQ, GC = self._shape(H, KP), self._shape(H, KQ), self._shape(H, KP // 2 + KQ // 2)
        assert llks_p.dtype == torch.float64 and llks_p.is_contiguous() and llks_p.numel() % GP == 0
        R = llks_p.numel() // GP
        assert llks_q.dtype == torch.float64 and llks_q.is_contiguous() and llks_q.numel() == R * GQ
        n = 0
        if llks_c is not None and llks_c.numel():
            assert llks_c.dtype == torch.float64 and llks_c.is_contiguous() and R > 0 and llks_c.numel() % (R * GC) == 0
            n = llks_c.numel() // (R * GC)
        d_fr = self._tensor(freqs, torch.float64, np.float64)
        assert d_fr.dim() == 2 and int(d_fr.shape[0]) == R and int(d_fr.shape[1]) >= H
        errs, Fs = [], []
        for e in gamete_error:
            e = np.array(np.broadcast_to(np.asarray(e, dtype=np.float64), (R,)))
            if not np.all((e >= 0.0) & (e <= 1.0)):
                raise ValueError("gamete_error: every e must lie in [0, 1]")
            errs.append(torch.from_numpy(e).to(dev))
        for F in (inbreeding_p, inbreeding_q):
            if F is not None:
                F = np.array(np.broadcast_to(np.asarray(F, dtype=np.float64), (R,)))
                if not np.all((F >= 0.0) & (F < 1.0)):   # (False for NaN and infinities too)
                    raise ValueError("inbreeding: every F must lie in [0, 1)")
                F = torch.from_numpy(F).to(dev)
            Fs.append(F)
        d_reads = None
        if progeny_reads is not None and n:
            reads = np.ascontiguousarray(progeny_reads, dtype=np.int32)
            assert reads.shape == (R, n)
            d_reads = torch.from_numpy(reads).to(dev)
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)          # noqa: E731
        i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)            # noqa: E731
        out = dict(post_p=f64(R, GP), post_q=f64(R, GQ), mode_p=i64(R), mode_q=i64(R), prob_p=f64(R), prob_q=f64(R), log_z=f64(R),
                   mode_c=i64(R, n), prob_c=f64(R, n), pred=f64(R, n))
        if R == 0:
            if full:
                out["q"] = f64(0, n, GC)
            return out
        wsb = self.workspace_bytes(R, H, KP, KQ, force_fallback)
        free, _ = torch.cuda.mem_get_info()
        limit = free if workspace_limit is None else min(int(workspace_limit), free)
        if wsb < 0 or wsb + (R * n * GC * 8 if full else 0) > limit:
            raise NotImplementedError("mchap_hip: family of %d records, ploidies %d x %d over %d haplotypes: the shape is refused, or "
                                      "its [G_P][G_Q] workspace is beyond what is offered" % (R, KP, KQ, H))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        if full:
            out["q"] = f64(R, n, GC)
        _lib.check(_lib.lib().mchap_exact_family_device(
            R, n, _ptr(llks_p), _ptr(llks_q), _ptr(llks_c) if n else None, _ptr(d_reads), H, KP, KQ, _ptr(Fs[0]), _ptr(Fs[1]),
            _ptr(d_fr), int(d_fr.shape[1]), _ptr(errs[0]), _ptr(errs[1]), _ptr(out["post_p"]), _ptr(out["mode_p"]), _ptr(out["prob_p"]),
            _ptr(out["post_q"]), _ptr(out["mode_q"]), _ptr(out["prob_q"]), _ptr(out["q"]) if full else None,
            _ptr(out["mode_c"]) if n else None, _ptr(out["prob_c"]) if n else None, _ptr(out["pred"]) if n else None, _ptr(out["log_z"]),
            _ptr(ws), C.c_int64(wsb), 1 if force_fallback else 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.launches += 1
        return out


class DenovoRaggedBatch(_OwnBuffers):
    """Units of different shapes (loci with different numbers of SNVs and alleles, samples with different read depths,
    per-sample ploidy / inbreeding) in ONE sampler launch, with the posterior summary and the replicate incongruence
    taken on the device: what `mchap assemble` needs per (locus x sample) comes back as a few hundred bytes per unit.

    units: list of dicts with reads float64 [R, M, A] (R >= 1, M >= 1), counts int64 [R] or None, n_alleles int [M],
    ploidy int, inbreeding float or None, stream_id int.  Sampler settings from `model` (a DenovoMCMC; its ploidy /
    n_alleles / inbreeding fields are not used)."""

    n_runs = 0  # sampler launches issued by this class (the application tests assert O(1) per VCF)

    def __init__(self, model: DenovoMCMC, units, device=None):
        torch = _torch()
        self.torch = torch
        self.device = dev = _device(torch, device)
        self.model = model
        U = len(units)
        Cn, S = int(model.chains), int(model.steps)
        self.Cn, self.S = Cn, S
        desc = np.zeros(U, dtype=_lib.UNIT_DTYPE)
        r_parts, c_parts, a_parts = [], [], []
        r_off = c_off = a_off = t_off = l_off = f_off = 0
        self.Kmax = max(int(u["ploidy"]) for u in units)
        self.max_pos = max(u["reads"].shape[1] for u in units)
        for i, u in enumerate(units):
            rd = np.ascontiguousarray(u["reads"], dtype=np.float64)
            R, M, A = rd.shape
            assert R >= 1 and M >= 1 and len(u["n_alleles"]) == M
            K = int(u["ploidy"])
            D = desc[i]
            D["reads_off"] = r_off
            r_parts.append(rd.reshape(-1))
            r_off += rd.size
            if u.get("counts") is not None:
                cn = np.ascontiguousarray(u["counts"], dtype=np.int64)
                assert cn.shape == (R,)
                D["counts_off"] = c_off
                c_parts.append(cn)
                c_off += R
            else:
                D["counts_off"] = -1
            D["nalleles_off"] = a_off
            a_parts.append(np.asarray(u["n_alleles"], dtype=np.int8))
            a_off += M
            D["initial_off"] = -1
            D["trace_off"] = t_off
            t_off += Cn * S * K
            D["llk_off"] = l_off
            l_off += Cn * S
            D["fixed_off"] = f_off
            f_off += M
            D["n_reads"], D["n_pos"], D["max_allele"], D["ploidy"] = R, M, A, K
            F = u.get("inbreeding")
            D["inbreeding"] = np.nan if F is None else float(F)
            D["stream_id"] = int(u.get("stream_id", 0))
        self._allocate(desc, t_off, l_off, f_off)   # (refuses before anything large is uploaded)
        self.d_reads = torch.from_numpy(np.concatenate(r_parts)).to(dev)
        self.d_counts = torch.from_numpy(np.concatenate(c_parts)).to(dev) if c_parts else None
        self.d_nalleles = torch.from_numpy(np.concatenate(a_parts)).to(dev)

    @classmethod
    def from_calls(cls, model, calls, reads_off, n_reads, n_pos, max_allele, ploidy, counts, counts_off, n_alleles, nalleles_off,
                   inbreeding=None, error_rate=0.0024, device=None, quals=None):
        """The same batch from the compact input (reference encoders: encoding/integer/transcode.py:16-77 with base qualities
        ignored, as the programs do by default), built with array operations only -- one row of every array per unit:
        calls int8 (all units' [n_reads, n_pos] matrices of allele calls, < 0 = gap, unit u at reads_off[u]), counts int64 (unit u's
        n_reads[u] counts at counts_off[u]; -1 = none), n_alleles int8 (unit u's n_pos[u] values at nalleles_off[u]; units may
        share them), inbreeding float [U] (NaN = none) or None.  quals: None, or -- base qualities in use -- int16 laid out like calls:
        a called cell of quality q then gives its allele prob_of_qual(q) * (1 - error_rate) (reference io/bam.py:280-288), read on
        the device from a table of as many entries as the largest quality asks for."""
        self = cls.__new__(cls)
        torch = _torch()
        self.torch = torch
        self.device = dev = _device(torch, device)
        self.model = model
        n_reads, n_pos, ploidy = (np.asarray(x, dtype=np.int64) for x in (n_reads, n_pos, ploidy))
        U = len(n_reads)
        Cn, S = int(model.chains), int(model.steps)
        self.Cn, self.S = Cn, S
        assert U and (n_reads >= 1).all() and (n_pos >= 1).all()
        desc = np.zeros(U, dtype=_lib.UNIT_DTYPE)
        desc["reads_off"], desc["counts_off"], desc["nalleles_off"] = reads_off, counts_off, nalleles_off
        desc["initial_off"] = -1
        t = Cn * S * ploidy
        desc["trace_off"] = np.cumsum(t) - t
        desc["llk_off"] = np.arange(U, dtype=np.int64) * (Cn * S)
        desc["fixed_off"] = np.cumsum(n_pos) - n_pos
        desc["n_reads"], desc["n_pos"], desc["max_allele"], desc["ploidy"] = n_reads, n_pos, max_allele, ploidy
        desc["inbreeding"] = np.nan if inbreeding is None else inbreeding
        desc["stream_id"] = 0
        self.Kmax, self.max_pos = int(ploidy.max()), int(n_pos.max())
        self._allocate(desc, t.sum(), U * Cn * S, n_pos.sum())
        self._upload_compact(calls, quals, error_rate, reject_negative="DenovoRaggedBatch.from_calls")
        self.d_counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).to(dev) if len(counts) else None
        self.d_nalleles = torch.from_numpy(np.ascontiguousarray(n_alleles, dtype=np.int8)).to(dev)
        return self

    def _host_summary(self, u, st, fixed, cache):
        """The summary of unit u by the host classes on its downloaded traces (assemble/classes.py:280-376 as the reference runs
        them): only for a unit whose chains visited more distinct genotypes than even the listed launch's LDS table holds --
        tens of thousands of steps.  cache: dict holding the batch's traces once most of its units come this way."""
        from .classes import GenotypeMultiTrace

        D = self.units_host[u]
        Ku, M, A, W = int(D["ploidy"]), int(D["n_pos"]), int(D["max_allele"]), self.wph
        fx = fixed[int(D["fixed_off"]): int(D["fixed_off"]) + M]

        def piece(name, dev, lo, n, view=None):
            if cache.get("whole"):
                if name not in cache:
                    a = dev.cpu().numpy()
                    cache[name] = a.view(view) if view is not None else a
                return cache[name][lo: lo + n]
            a = dev[lo: lo + n].cpu().numpy()
            return a.view(view) if view is not None else a

        w = piece("trace", self.d_trace, int(D["trace_off"]), self.Cn * self.S * Ku * W, np.uint64)
        w = w.reshape((self.Cn, self.S, Ku) + ((W,) if W > 1 else ()))
        g = unpack_trace(w, fx, A, W)
        lk = piece("llks", self.d_llks, int(D["llk_off"]), self.Cn * self.S).reshape(self.Cn, self.S)
        tr = GenotypeMultiTrace._from_sorted(g, lk).burn(self.burn)
        post = tr.posterior()
        sup = post.mode_genotype_support()
        mg, gp = sup.mode_genotype()
        return dict(genotypes=post.genotypes, probabilities=post.probabilities, spm=float(sup.probabilities.sum()), gpm=float(gp),
                    mode_genotype=mg, mci=int(tr.replicate_incongruence(self.incongruence_threshold)), status=st)

    def run(self, burn, max_states=512, incongruence_threshold=0.6):
        """Sampler, posterior summary and incongruence code, all enqueued on torch's current stream."""
        torch = self.torch
        dev = self.device
        U, K, W = self.n_units, self.Kmax, self.wph  # (W = 2: a batch of the general sampler, two words per haplotype -- round 5)
        stream = self._begin().cuda_stream
        L = _lib.lib()
        type(self).n_runs += 1
        self._fit(stream)
        self.max_states = max_states
        if W > 1:  # (wider states: the batch launch's table is what the LDS holds of them)
            max_states = min(int(max_states), int(L.mchap_trace_posterior_max_states_wph(K, W)))
            self.max_states = max_states
        self.p_words = torch.empty(U * max_states * K * W, dtype=torch.int64, device=dev)
        self.p_counts = torch.empty(U * max_states, dtype=torch.int32, device=dev)
        self.p_n = torch.empty(U, dtype=torch.int32, device=dev)
        self.p_stats = torch.empty(U * 2, dtype=torch.float64, device=dev)
        self.p_mode = torch.empty(U, dtype=torch.int32, device=dev)
        self.p_mode_words = torch.empty(U * K * W, dtype=torch.int64, device=dev)
        self.p_mode_count = torch.empty(U, dtype=torch.int32, device=dev)
        self.p_mci = torch.empty(U, dtype=torch.int32, device=dev)
        _lib.check(L.mchap_trace_posterior_batch_wph_device(
            U, _ptr(self.d_units), self.S, self.Cn, int(burn), _ptr(self.d_trace), int(max_states), K, W, _ptr(self.p_words),
            _ptr(self.p_counts), _ptr(self.p_n), _ptr(self.p_stats), _ptr(self.p_mode), _ptr(self.p_mode_words),
            _ptr(self.p_mode_count), C.c_void_p(stream)))
        _lib.check(L.mchap_trace_incongruence_batch_wph_device(
            U, _ptr(self.d_units), self.S, self.Cn, int(burn), _ptr(self.d_trace), K, W, C.c_double(float(incongruence_threshold)),
            _ptr(self.p_mci), C.c_void_p(stream)))
        self.burn = int(burn)
        self.incongruence_threshold = float(incongruence_threshold)
        self._end()

    def _summarise_listed(self, over):
        """The units `over` (int32 indices) summarised again with a table of chains x (steps - burn) states (as many as the LDS
        holds): their entries of p_n / p_stats / p_mode_words / p_mci are rewritten; returns (words int64 [len(over) * cap * K * wph],
        counts int32 [len(over) * cap] on the device, cap)."""
        torch = self.torch
        L = _lib.lib()
        K, W = self.Kmax, self.wph
        total = self.Cn * (self.S - self.burn)
        cap = min(total, int(L.mchap_trace_posterior_max_states_wph(K, W)))
        stream = torch.cuda.current_stream().cuda_stream
        d_list = torch.from_numpy(np.ascontiguousarray(over, dtype=np.int32)).to(self.device)
        o_words = torch.empty(len(over) * cap * K * W, dtype=torch.int64, device=self.device)
        o_counts = torch.empty(len(over) * cap, dtype=torch.int32, device=self.device)
        _lib.check(L.mchap_trace_posterior_listed_wph_device(
            len(over), _ptr(d_list), _ptr(self.d_units), self.S, self.Cn, self.burn, _ptr(self.d_trace), cap, K, W,
            _ptr(o_words), _ptr(o_counts), _ptr(self.p_n), _ptr(self.p_stats), _ptr(self.p_mode),
            _ptr(self.p_mode_words), _ptr(self.p_mode_count), C.c_void_p(stream)))
        _lib.check(L.mchap_trace_incongruence_listed_wph_device(
            len(over), _ptr(d_list), _ptr(self.d_units), self.S, self.Cn, self.burn, _ptr(self.d_trace),
            min(self.S - self.burn, cap), K, W, C.c_double(self.incongruence_threshold), _ptr(self.p_mci), C.c_void_p(stream)))
        return o_words, o_counts, cap

    def _summary_state(self, only=None):
        """The summaries of run() on the host, but for the tables of distinct genotypes (they stay on the device: p_words / p_counts,
        and the listed launch's): (dict(n, stats [U, 2], mode_words [U, K] + two-word axis, mci, status, fixed, total), over, (o_words,
        o_counts, cap)).  over: the units -- of `only`, by default of all -- whose chains visited more distinct genotypes than the
        batch kernels keep (samples with few or no reads: their chains wander); they are summarised again on the device with a
        table that cannot overflow, a list launch over those units only (_summarise_listed: its result, or (None, None, max_states)
        without such units), and the dict holds what it rewrote -- no trace is downloaded, no posterior formed on the host."""
        U, K, ms, W = self.n_units, self.Kmax, self.max_states, self.wph
        self._begin()  # (the pass may have been issued on another stream)
        status, n, mci = self.d_status.cpu().numpy(), self.p_n.cpu().numpy(), self.p_mci.cpu().numpy()
        over = np.flatnonzero((status >= 0) & ((n < 0) | (n > ms) | (mci < 0))).astype(np.int32)
        if only is not None:
            over = np.intersect1d(over, np.asarray(only, dtype=np.int32)).astype(np.int32)
        listed = (None, None, ms)
        if len(over):
            listed = self._summarise_listed(over)
            n, mci = self.p_n.cpu().numpy(), self.p_mci.cpu().numpy()
        state = dict(n=n, stats=self.p_stats.cpu().numpy().reshape(U, 2),
                     mode_words=self.p_mode_words.cpu().numpy().view(np.uint64).reshape((U, K) + ((W,) if W > 1 else ())),
                     mci=mci, status=status, fixed=self.d_fixed.cpu().numpy(), total=self.Cn * (self.S - self.burn))
        return state, over, listed

    def summary_arrays(self):
        """The posterior summaries of all units as arrays (what results() turns into one dict per unit): dict(n [U] distinct
        genotypes of each unit, plain [U] bool: the unit's summary is complete in these arrays -- the others (more distinct
        states than max_states, beyond a limit) go through results(only=...); words uint64 [N, K] / counts int32 [N]: the
        packed distinct genotypes of the plain units, unit after unit, most probable first (N = n[plain].sum(): only these
        rows leave the device; [N, K, 2] / [U, K, 2] for a batch of the general sampler: two words per haplotype); stats float64 [U, 2]
        (SPM, GPM), mode_words uint64 [U, K], mci [U], status [U], fixed int8
        flat (unit u at units_host['fixed_off'][u]), total = the steps a probability is a count of)."""
        torch = self.torch
        U, K, ms, Wp = self.n_units, self.Kmax, self.max_states, self.wph
        KW = K * Wp   # words of a state (a batch of the general sampler: two words per haplotype, the more significant first)
        wshape = (Wp,) if Wp > 1 else ()
        # (the units the listed launch summarised again: their rows are taken from its table)
        out, over, (o_words, o_counts, cap) = self._summary_state()
        n, mci, status = out["n"], out["mci"], out["status"]
        is_over = np.zeros(U, dtype=bool)
        is_over[over] = True
        out["plain"] = (status >= 0) & (n >= 0) & (n <= np.where(is_over, cap, ms)) & (mci >= 0)
        nn = np.where(out["plain"], n, 0).astype(np.int64)
        first = np.cumsum(nn) - nn                         # where each unit's rows start in the ragged result

        def gather(sel, table_row, words, counts):
            """rows of the units `sel` (indices): unit k's rows start at table_row[k] of the device table"""
            k_ = nn[sel]
            rows = np.repeat(table_row - (np.cumsum(k_) - k_), k_) + np.arange(int(k_.sum()), dtype=np.int64)
            d_rows = torch.from_numpy(rows).to(self.device)
            return words.view(-1, KW)[d_rows].cpu().numpy().view(np.uint64), counts[d_rows].cpu().numpy(), np.repeat(first[sel] - (np.cumsum(k_) - k_), k_) + np.arange(int(k_.sum()), dtype=np.int64)

        N = int(nn.sum())
        W, Cc = np.empty((N, KW), dtype=np.uint64), np.empty(N, dtype=np.int32)
        reg = np.flatnonzero(~is_over)
        w_, c_, dst = gather(reg, reg.astype(np.int64) * ms, self.p_words, self.p_counts)
        W[dst], Cc[dst] = w_, c_
        if len(over):
            w_, c_, dst = gather(over.astype(np.int64), np.arange(len(over), dtype=np.int64) * cap, o_words, o_counts)
            W[dst], Cc[dst] = w_, c_
        out["words"], out["counts"] = W.reshape((N, K) + wshape), Cc
        return out

    def results(self, raise_on_limit=True, only=None):
        """(only: the units to report, default all.)  Per unit: dict(genotypes int8 [n, K, M] distinct states (probability descending), probabilities [n], spm, gpm,
        mode_genotype int8 [K, M], mci, status).  Units with more distinct states than the batch kernels keep (512) are
        summarised by a second, listed launch with a table of chains x (steps - burn) states (as many as the LDS holds).
        A unit beyond the library's packed haplotype width raises NotImplementedError, or with raise_on_limit=False comes
        back as dict(status, limit=reason)."""
        U, K, ms, W = self.n_units, self.Kmax, self.max_states, self.wph
        wshape = (W,) if W > 1 else ()   # (a haplotype of a wide batch is two words: unpack_trace(..., W))
        state, over, (o_words, o_counts, cap) = self._summary_state(only)
        n, stats, mode_words, mci, status, fixed, total = (state[k] for k in ("n", "stats", "mode_words", "mci", "status", "fixed", "total"))
        words = self.p_words.cpu().numpy().view(np.uint64).reshape((U, ms, K) + wshape)
        counts = self.p_counts.cpu().numpy().reshape(U, ms)
        over_row = {}
        if len(over):
            ow = o_words.cpu().numpy().view(np.uint64).reshape((len(over), cap, K) + wshape)
            oc = o_counts.cpu().numpy().reshape(len(over), cap)
            over_row = {int(u): (ow[i], oc[i], cap) for i, u in enumerate(over)}
        out = []
        wanted = range(U) if only is None else only
        host_cache = {"whole": 4 * len(wanted) >= U}  # (traces for _host_summary: the batch's at once, or a unit's slice at a time)
        for u in wanted:
            D = self.units_host[u]
            Ku, M, A = int(D["ploidy"]), int(D["n_pos"]), int(D["max_allele"])
            fx = fixed[int(D["fixed_off"]): int(D["fixed_off"]) + M]
            st = int(status[u])
            if st == _lib.UNIT_NAN_LLK:
                raise ValueError("Encountered log likelihood of nan")
            if st == _lib.UNIT_BREAKS:
                raise ValueError("breaks must be smaller then n")
            if st < 0:
                if raise_on_limit:
                    raise NotImplementedError("mchap_hip: unit %d exceeds the packed haplotype width" % u)
                out.append(dict(status=st, limit="more than %d bits of sampled alleles per haplotype (one bit per biallelic, two per "
                                                 "tri- / tetra-allelic SNV that is not fixed as homozygous)" % (128 if W > 1 else 64)))
                continue
            if u in over_row and 0 <= n[u] <= over_row[u][2] and mci[u] >= 0:
                w_, c_, _ = over_row[u]
                k = int(n[u])
                out.append(dict(genotypes=unpack_trace(w_[:k, :Ku], fx, A, W), probabilities=c_[:k] / total, spm=float(stats[u, 0]),
                                gpm=float(stats[u, 1]), mode_genotype=unpack_trace(mode_words[u, :Ku], fx, A, W), mci=int(mci[u]), status=st))
                continue
            if n[u] < 0 or n[u] > ms or mci[u] < 0:
                # (more distinct states than even the LDS holds -- tens of thousands of steps: the host classes on the trace)
                out.append(self._host_summary(u, st, fixed, host_cache))
                continue
            k = int(n[u])
            out.append(dict(genotypes=unpack_trace(words[u, :k, :Ku], fx, A, W), probabilities=counts[u, :k] / total,
                            spm=float(stats[u, 0]), gpm=float(stats[u, 1]), mode_genotype=unpack_trace(mode_words[u, :Ku], fx, A, W),
                            mci=int(mci[u]), status=st))
        return out
