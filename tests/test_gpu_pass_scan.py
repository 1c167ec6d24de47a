"""The list scan every priority pass starts with (pass_scan, fim_kernels.hip): the
16 shard counts' inclusive prefix, the 64-bin inclusive prefix of the histogram
summed over the shards, the target / cap arithmetic and the threshold bin b*.
dymu_pass_scan_probe runs it in one wave on given inputs; the reference is a numpy
cumsum restatement, compared exactly.

The scan moves data between lanes in 16-lane rows (bins 0-15, 16-31, 32-47, 48-63)
and then from row to row, so b* is placed on both sides of every row boundary."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF


def scan_ref(counts, hist, target, target_frac, cap_frac):
    """(prefix[0..16], b*) as the kernels define them (sums mod 2^32, f32 fractions)."""
    m32 = np.uint64(M32)
    prefix = np.zeros(17, dtype=np.uint64)
    prefix[1:] = np.cumsum(counts.astype(np.uint64)) & m32
    n = int(prefix[16])
    hp = np.cumsum(hist.astype(np.uint64).sum(axis=0) & m32) & m32
    t = max(target, int(np.float32(target_frac) * np.float32(n)))
    if cap_frac > 0.0:
        t = min(t, max(int(np.float32(cap_frac) * np.float32(n)), 256))
    reach = [b for b in range(63) if int(hp[b]) >= t]
    bstar = reach[0] if target > 0 and n > t and reach else 64
    return prefix.astype(np.uint32), bstar


def spread(rng, total):
    """`total` split over the 16 shards."""
    cuts = np.sort(rng.integers(0, total + 1, 15))
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.uint32)


def check(engine, counts, hist, target, target_frac=0.0, cap_frac=0.0, want_bstar=None):
    counts = np.asarray(counts, dtype=np.uint32)
    hist = np.asarray(hist, dtype=np.uint32)
    prefix, bstar = engine.pass_scan_probe(counts, hist, target, target_frac, cap_frac)
    ref_prefix, ref_bstar = scan_ref(counts, hist, target, target_frac, cap_frac)
    if want_bstar is not None:
        assert ref_bstar == want_bstar  # the case is what its name says
    assert np.array_equal(prefix, ref_prefix)
    assert bstar == ref_bstar


def at_bin(rng, b, target=1000):
    """A list of 3,499 tiles whose histogram prefix is target - 1 up to bin b - 1 and
    passes the target in bin b; the tail sits in bin 63, which never counts."""
    hist = np.zeros((16, 64), dtype=np.uint32)
    if b > 0:
        lo = rng.integers(0, b, target - 1)
        lo[0] = b - 1  # the bin next to b* holds a tile
        np.add.at(hist, (rng.integers(0, 16, lo.size), lo), 1)
    hist[:, b] += spread(rng, 500 if b > 0 else target + 499)
    hist[:, 63] += spread(rng, 2000)
    return hist.sum(axis=1).astype(np.uint32), hist


@pytest.mark.parametrize("b", [0, 1, 15, 16, 17, 31, 32, 47, 48, 62])
def test_bstar_at_bin(engine, b):
    counts, hist = at_bin(np.random.default_rng(100 + b), b)
    check(engine, counts, hist, 1000, want_bstar=b)


def test_no_bin_reaches_the_target(engine):
    rng = np.random.default_rng(1)
    hist = np.zeros((16, 64), dtype=np.uint32)
    hist[:, 5] = spread(rng, 300)
    hist[:, 63] = spread(rng, 5000)  # bin 63 is never a threshold
    check(engine, hist.sum(axis=1), hist, 1000, want_bstar=64)


@pytest.mark.parametrize("n", [999, 1000])
def test_list_no_longer_than_the_target(engine, n):
    rng = np.random.default_rng(2)
    hist = np.zeros((16, 64), dtype=np.uint32)
    hist[:, 3] = spread(rng, n)
    check(engine, hist.sum(axis=1), hist, 1000, want_bstar=64)


def test_cap_binds(engine):
    """1,000 listed, target 1,000: without the cap every tile is relaxed (b* = 64); the
    90 % cap lowers the target to 900, reached in bin 5."""
    rng = np.random.default_rng(3)
    hist = np.zeros((16, 64), dtype=np.uint32)
    hist[:, 4] = spread(rng, 899)
    hist[:, 5] = spread(rng, 50)
    hist[:, 40] = spread(rng, 51)
    counts = hist.sum(axis=1)
    check(engine, counts, hist, 1000, cap_frac=0.0, want_bstar=64)
    check(engine, counts, hist, 1000, cap_frac=0.9, want_bstar=5)


def test_cap_floor_of_256_tiles(engine):
    """200 listed: 90 % is 180, which bin 3 reaches, but the cap is not below 256 tiles,
    more than the list holds: every tile is relaxed."""
    rng = np.random.default_rng(4)
    hist = np.zeros((16, 64), dtype=np.uint32)
    hist[:, 3] = spread(rng, 190)
    hist[:, 9] = spread(rng, 10)
    check(engine, hist.sum(axis=1), hist, 1000, cap_frac=0.9, want_bstar=64)
    # 280 listed: 90 % is 252, the floor of 256 is the target; bin 3 holds 250, bin 9 260
    hist[:, 2] = spread(rng, 60)
    hist[:, 50] = spread(rng, 20)
    check(engine, hist.sum(axis=1), hist, 1000, cap_frac=0.9, want_bstar=9)


def test_all_zero(engine):
    check(engine, np.zeros(16), np.zeros((16, 64)), 1000, cap_frac=0.9, want_bstar=64)


@pytest.mark.parametrize("shard", [0, 15])
def test_single_shard(engine, shard):
    counts = np.zeros(16, dtype=np.uint32)
    counts[shard] = 4000
    hist = np.zeros((16, 64), dtype=np.uint32)
    hist[shard, 20] = 1500
    hist[shard, 21] = 2500
    check(engine, counts, hist, 1000, cap_frac=0.9, want_bstar=20)


def test_counts_near_2_to_31(engine):
    """Totals just below 2^31: the prefixes and the f32 fraction arithmetic at that size."""
    rng = np.random.default_rng(5)
    counts = np.full(16, (1 << 27) - 3, dtype=np.uint32)
    hist = np.zeros((16, 64), dtype=np.uint32)
    hist[:, 16] = (1 << 26) - 1  # 2^30 - 16 in all: one short of ...
    hist[:, 33] = rng.integers(1, 1000, 16)  # ... the half of the list reached here
    hist[:, 63] = counts - hist[:, 16] - hist[:, 33]
    check(engine, counts, hist, 14 * 256, target_frac=0.5, want_bstar=33)
    check(engine, counts, hist, 14 * 256, target_frac=0.5, cap_frac=0.9, want_bstar=33)
    check(engine, counts, hist, 1 << 30, want_bstar=33)


def test_target_zero(engine):
    counts, hist = at_bin(np.random.default_rng(6), 17)
    check(engine, counts, hist, 0, want_bstar=64)
    check(engine, counts, hist, 0, target_frac=0.25, cap_frac=0.9, want_bstar=64)


@pytest.mark.parametrize("seed", range(4))
def test_random(engine, seed):
    """Dense random histograms: every lane of every row carries a value."""
    rng = np.random.default_rng(50 + seed)
    hist = rng.integers(0, 200, (16, 64)).astype(np.uint32)
    counts = hist.sum(axis=1).astype(np.uint32)
    for target in (1, 3584, 50000, int(counts.sum())):
        check(engine, counts, hist, target, target_frac=0.01 * seed, cap_frac=0.9 if seed & 1 else 0.0)
