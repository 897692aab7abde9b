"""The kernels of the expected allele depths -- exact_support_kernel<8|16>, exact_support_combine_kernel, after the evidence
launches for the normaliser -- driven through device.ExactReadSupport on the library's own float64 likelihoods of drawn read
tensors, against the long-double reference (tests/allele_support_reference.py; tests/test_allele_support_reference.py anchors it on
the CPU).  The bound: |got - want| <= 1e-9 |want| + (8 x ENVELOPE) x N, N the unit's read weight.  Shapes: 1, 63, 65 and 130 read
rows, the genotype tile's edge, both KM instantiations' edge, ploidy 15, several read tiles with a ragged last one, a refused
shape; the flat prior, F = 0 with a zero frequency and F > 0; padding rows, a unit of all-zero weights, error-free reads, a unit
without a finite genotype, the per-read rows, and equal bits under a permutation of the batch."""
import functools
import zlib
from math import comb

import numpy as np
import pytest

from tests import allele_support_reference as ref

pytestmark = pytest.mark.gpu

A = 3
# name: (K, H, read rows)
SHAPES = {
    "rows-1": (4, 5, 1),
    "rows-63": (4, 5, 63),
    "rows-65": (4, 5, 65),
    "rows-130": (4, 5, 130),
    "tile-less-one": (2, 90, 7),
    "tail-of-90": (2, 91, 7),
    "last-of-KM8": (8, 8, 6),
    "first-of-KM16": (9, 8, 6),
    "K15-H6": (15, 6, 5),
    "read-tiles": (2, 40, 300),
}
F_POSITIVE = 0.3


def support_lds_bytes(H, K, RT):
    """exact_support_lds (exact_support_kernel.hpp), restated: the staging tile, the runs' first genotypes, the prior tables, the
    depth sums, the tile's weights, P and the accumulator."""
    return (256 * 17 + 256 * 2 + H * (K + 1) + (K + 1) + 2 * H + 1 + RT + 2 * H * RT) * 8


def support_tile(R, H, K):
    """exact_support_rows, restated: the largest multiple of 64 within the reads' need and 64 KB; one tile of 64 up to 160 KB."""
    rt = 0
    if H > 255:
        return 0
    while rt + 64 <= (R + 63) // 64 * 64 and support_lds_bytes(H, K, rt + 64) <= 64 * 1024:
        rt += 64
    if rt == 0 and support_lds_bytes(H, K, 64) <= 160 * 1024:
        rt = 64
    return rt


def positions(H):
    m = 4
    while A ** m < 2 * H:
        m += 1
    return m


@functools.lru_cache(maxsize=None)
def shape_inputs(name, error_free=False):
    """(haps int8 [H, M], freqs float64 [2, H] -- row 0 with a zero frequency --, [(dists, counts)] of three units)."""
    K, H, R = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(("gpu-support-%s-%d" % (name, error_free)).encode()))
    haps = ref.draw_haplotypes(rng, H, positions(H), A)
    freqs = rng.dirichlet(np.full(H, 2.0), size=2)
    freqs[0, 1 % H] = 0.0
    freqs[0] /= freqs[0].sum()
    units = [ref.draw_reads(rng, haps, R, A, error_free=error_free) for _ in range(3)]
    return haps, freqs, units


def run(K, haps, units, Fs, rows, freqs, per_read=False, llks=None):
    """device.ExactReadSupport.add_group over the units [(dists, counts)] -> (depth [U, H], read_post [U, R, H] or None, the
    library's llks64 [U, G], log_norm [U]) on the host.  llks: tables to use in place of the library's own."""
    import torch

    from mchap_amd.device import ExactDeviceBatch, ExactReadSupport

    reads = np.stack([d for d, _ in units])
    counts = np.stack([c for _, c in units])
    batch = ExactDeviceBatch(reads, K, haps, counts, None, cache_joint=False)
    own = batch.run_llks64()
    if llks is not None:
        own = torch.from_numpy(np.ascontiguousarray(np.concatenate(llks))).to(batch.device)
    support = ExactReadSupport(batch.device)
    got = support.add_group(batch, own, Fs, rows, freqs, per_read=per_read)
    torch.cuda.synchronize()
    depth, post = got if per_read else (got, None)
    return (depth.cpu().numpy(), None if post is None else post.cpu().numpy(), own.cpu().numpy().reshape(len(units), -1),
            support.log_norm.cpu().numpy())


def check_unit(depth, post, unit, haps, llk, K, F, f):
    """The unit's arrays against the long-double reference on the same likelihoods -> the largest deviations."""
    dists, counts = unit
    N = float(counts.sum())
    want_depth, want_post = ref.support(dists, counts, haps, llk, K, F, f)
    ok, err = ref.within(depth, want_depth, N)
    assert ok, ("depth", err, ref.floor(N))
    if not np.isnan(want_depth[0]):
        assert abs(depth.sum() - want_depth.sum()) <= ref.REL * N + ref.floor(N) * len(depth)
    if post is not None:
        okp, errp = ref.within(post, want_post, 1.0)
        assert okp, ("read_post", errp, ref.floor(1.0))
        err = max(err, errp)
    return err


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_kernels_against_long_double(name):
    from mchap_amd import _lib

    K, H, R = SHAPES[name]
    haps, freqs, units = shape_inputs(name)
    assert int(_lib.lib().mchap_exact_support_tile(R, H, K)) == support_tile(R, H, K) > 0
    # F = 0 with a zero frequency and F > 0 in one launch; then the flat prior
    depth, _, llks, norm = run(K, haps, units[:2], [0.0, F_POSITIVE], [0, 1], freqs)
    worst = max(check_unit(depth[0], None, units[0], haps, llks[0], K, 0.0, freqs[0]),
                check_unit(depth[1], None, units[1], haps, llks[1], K, F_POSITIVE, freqs[1]))
    assert depth[0, 1 % H] == 0.0 or H == 1       # the allele of frequency 0 carries no read
    assert np.all(np.isfinite(norm))
    flat, _, llks, _ = run(K, haps, units[2:], None, None, None)
    worst = max(worst, check_unit(flat[0], None, units[2], haps, llks[0], K, None, None))
    print("%s: worst |deviation| %.3g (REL %g, FLOOR per unit of weight %.3g)" % (name, worst, ref.REL, ref.floor(1.0)))


def test_the_read_tiles_are_ragged_and_the_refused_shape_raises():
    from mchap_amd import _lib
    from mchap_amd.device import ExactDeviceBatch, ExactReadSupport

    L = _lib.lib()
    K, H, R = SHAPES["read-tiles"]
    tile = int(L.mchap_exact_support_tile(R, H, K))
    assert tile == 64 and R // tile >= 2 and R % tile != 0          # several tiles, the last one partial
    assert int(L.mchap_exact_support_tile(130, 5, 4)) == 192          # (as many rows as the reads need, within 64 KB)
    assert int(L.mchap_exact_support_tile(10, 500, 2)) == 0 and support_tile(10, 500, 2) == 0
    assert int(L.mchap_exact_support_tile(10, 5, 16)) == 0 and int(L.mchap_exact_support_tile(0, 5, 2)) == 0
    assert int(L.mchap_exact_support_workspace_bytes(1, 10, 5, 16, 0)) == -1
    rng = np.random.default_rng(2)
    haps = ref.draw_haplotypes(rng, 500, positions(500), A)
    dists, counts = ref.draw_reads(rng, haps, 10, A)
    batch = ExactDeviceBatch(dists[None], 2, haps, counts[None], None, cache_joint=False)
    support = ExactReadSupport(batch.device)
    with pytest.raises(NotImplementedError):
        support.add_group(batch, batch.run_llks64(), None, None, None)
    # F is checked on the host copy, before any launch
    haps, freqs, units = shape_inputs("rows-1")
    small = ExactDeviceBatch(units[0][0][None], 4, haps, units[0][1][None], None, cache_joint=False)
    for bad in (1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            support.add_group(small, small.run_llks64(), [bad], [0], freqs)
    assert support.launches == 0


def test_padding_rows_and_a_unit_of_zero_weights_in_a_mixed_batch():
    name = "rows-65"
    K, H, R = SHAPES[name]
    haps, freqs, units = shape_inputs(name)
    padded = (units[0][0].copy(), units[0][1].copy())
    padded[0][R - 10:] = np.nan                     # padding as the programs pad: all-gap rows of weight 0
    padded[1][R - 10:] = 0
    zero = (units[1][0], np.zeros(R, dtype=np.int64))
    batch = [padded, zero, units[2]]
    depth, post, llks, _ = run(K, haps, batch, [0.0, F_POSITIVE, F_POSITIVE], [0, 1, 1], freqs, per_read=True)
    assert np.all(depth[1] == 0.0) and np.all(post[1] == 0.0)
    assert np.all(post[0][R - 10:] == 0.0) and np.all(post[2][units[2][1] == 0] == 0.0)
    for u, (F, row) in enumerate(((0.0, 0), (F_POSITIVE, 1), (F_POSITIVE, 1))):
        check_unit(depth[u], post[u], batch[u], haps, llks[u], K, F, freqs[row])
    # the padded unit without its padding: the same depths to the bound (the likelihood groups the rows by four, so not the bits)
    short = (padded[0][:R - 10], padded[1][:R - 10])
    alone, _, llk_alone, _ = run(K, haps, [short], [0.0], [0], freqs)
    assert ref.within(depth[0], alone[0], float(short[1].sum()))[0]


def test_error_free_reads():
    name = "rows-65"
    K, H, R = SHAPES[name]
    haps, freqs, units = shape_inputs(name, error_free=True)
    assert any(np.any(d == 0.0) for d, _ in units)
    Fs, rows = [0.0, F_POSITIVE, F_POSITIVE], [1, 1, 0]
    depth, post, llks, norm = run(K, haps, units, Fs, rows, freqs, per_read=True)
    assert np.any(np.isinf(llks))                      # genotypes that cannot have given a read
    for u in range(3):
        check_unit(depth[u], post[u], units[u], haps, llks[u], K, Fs[u], freqs[rows[u]])


def test_a_unit_without_a_finite_genotype_and_its_neighbours():
    name = "rows-63"
    K, H, R = SHAPES[name]
    haps, freqs, units = shape_inputs(name)
    _, _, llks, _ = run(K, haps, units, None, None, None)
    tables = [llks[0], np.full(llks.shape[1], -np.inf), llks[2]]
    Fs, rows = [0.0, F_POSITIVE, F_POSITIVE], [0, 1, 1]
    depth, post, _, norm = run(K, haps, units, Fs, rows, freqs, per_read=True, llks=tables)
    assert np.all(np.isnan(depth[1])) and np.all(np.isnan(post[1])) and norm[1] == -np.inf
    keep = [0, 2]
    alone, alone_post, _, _ = run(K, haps, [units[i] for i in keep], [Fs[i] for i in keep], [rows[i] for i in keep], freqs, per_read=True,
                                  llks=[tables[i] for i in keep])
    assert not np.any(np.isnan(alone)) and depth[keep].tobytes() == alone.tobytes() and post[keep].tobytes() == alone_post.tobytes()
    check_unit(depth[1], post[1], units[1], haps, tables[1], K, Fs[1], freqs[1])


@pytest.mark.parametrize("name", ["rows-130", "read-tiles"])
def test_the_per_read_rows(name):
    K, H, R = SHAPES[name]
    haps, freqs, units = shape_inputs(name)
    Fs, rows = [0.0, F_POSITIVE, F_POSITIVE], [0, 1, 1]
    depth, post, llks, _ = run(K, haps, units, Fs, rows, freqs, per_read=True)
    plain, _, _, _ = run(K, haps, units, Fs, rows, freqs)
    for u, (dists, counts) in enumerate(units):
        N = float(counts.sum())
        check_unit(depth[u], post[u], units[u], haps, llks[u], K, Fs[u], freqs[rows[u]])
        # every row with a weight sums to 1 (H terms, each within the bound of a row), a row without is exactly 0
        assert np.all(np.abs(post[u][counts > 0].sum(axis=1) - 1.0) <= H * (ref.REL + ref.floor(1.0)))
        assert np.all(post[u][counts == 0] == 0.0)
        # depth is the weighted sum of the rows: the kernel adds the R terms in row order, numpy pairwise -- R roundings of at
        # most 2^-53 N each on either side
        assert np.all(np.abs(depth[u] - (counts[:, None] * post[u]).sum(axis=0)) <= 2 * R * 2.0 ** -53 * N)
        assert abs(depth[u].sum() - N) <= H * (ref.REL * N + ref.floor(N))
        # the depths without the rows (summed inside the workgroups, in another order) agree to the bound
        assert ref.within(plain[u], depth[u], N)[0]


@pytest.mark.parametrize("name", ["rows-130", "tail-of-90"])
def test_a_permuted_batch_gives_equal_bits(name):
    K, H, R = SHAPES[name]
    haps, freqs, units = shape_inputs(name)
    Fs, rows = [0.0, F_POSITIVE, F_POSITIVE], [0, 1, 0]
    base, base_post, _, _ = run(K, haps, units, Fs, rows, freqs, per_read=True)
    again, _, _, _ = run(K, haps, units, Fs, rows, freqs, per_read=True)
    assert again.tobytes() == base.tobytes()
    order = [2, 0, 1]
    got, got_post, _, _ = run(K, haps, [units[i] for i in order], [Fs[i] for i in order], [rows[i] for i in order], freqs, per_read=True)
    assert got.tobytes() == base[order].tobytes() and got_post.tobytes() == base_post[order].tobytes()
    plain, _, _, _ = run(K, haps, units, Fs, rows, freqs)
    shuffled, _, _, _ = run(K, haps, [units[i] for i in order], [Fs[i] for i in order], [rows[i] for i in order], freqs)
    assert shuffled.tobytes() == plain[order].tobytes()


def test_calling_allele_read_support():
    from mchap_amd import calling

    name = "rows-65"
    K, H, R = SHAPES[name]
    haps, freqs, units = shape_inputs(name)
    dists, counts = units[0]
    base, base_post, llks, _ = run(K, haps, units[:1], [F_POSITIVE], [1], freqs, per_read=True)
    depth, post = calling.allele_read_support(dists, K, haps, read_counts=counts, prior=(F_POSITIVE, freqs[1]), per_read=True)
    assert depth.tobytes() == base[0].tobytes() and post.tobytes() == base_post[0].tobytes()
    flat = calling.allele_read_support(dists, K, haps, read_counts=counts)
    check_unit(flat, None, units[0], haps, llks[0], K, None, None)
    assert np.all(calling.allele_read_support(dists[:0], K, haps) == 0.0)
