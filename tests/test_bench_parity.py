"""bench.py's whole-map parity block (oracle_parity): the headline map against the
oracle FMM's map of the same grid -- identical +inf mask, <= 1e-12 relative."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _maps(n=2500, seed=0):
    rng = np.random.default_rng(seed)
    To = rng.uniform(0, 5e4, (n, n))
    To[rng.random((n, n)) < 0.02] = np.inf
    return To.copy(), To


def test_identical_maps_pass():
    Tg, To = _maps()
    p = bench.oracle_parity(Tg, To)
    assert p["ok"] and p["max_rel"] == 0.0 and p["mismatched_cells"] == 0
    assert p["finite_cells"] == int(np.isfinite(To).sum())


def test_ulp_differences_pass_and_larger_fail():
    Tg, To = _maps(seed=1)
    Tg[5, 7] = np.nextafter(To[5, 7], np.inf) if np.isfinite(To[5, 7]) else Tg[5, 7]
    assert bench.oracle_parity(Tg, To)["ok"]
    j = np.argwhere(np.isfinite(To) & (To > 1))[0]
    Tg[j[0], j[1]] = To[j[0], j[1]] * (1 + 1e-10)
    p = bench.oracle_parity(Tg, To)
    assert not p["ok"] and 5e-11 < p["max_rel"] < 2e-10


def test_mask_mismatch_fails():
    Tg, To = _maps(seed=2)
    j = np.argwhere(np.isfinite(To))[0]
    Tg[j[0], j[1]] = np.inf
    p = bench.oracle_parity(Tg, To)
    assert not p["ok"] and p["mismatched_cells"] == 1


def test_sample_cells_whole_map_below_the_cap_fixed_sample_above():
    assert bench.sample_cells(1000, max_bytes=8000) is None  # fits: the whole map
    idx = bench.sample_cells(1001, max_bytes=8000)
    assert idx.dtype == np.int64 and 0 < idx.size <= 1000
    assert idx.min() >= 0 and idx.max() < 1001 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, bench.sample_cells(1001, max_bytes=8000))  # the same every time
    big = bench.sample_cells(16384 * 16384)
    assert big.size * 8 <= bench.DUMP_MAX_BYTES and big.max() < 16384 * 16384
    assert big.size > 0.99 * (bench.DUMP_MAX_BYTES // 8)  # few draws coincide


def test_dump_map_writes_float64_whole_or_sampled(tmp_path):
    idx = bench.sample_cells(60, 160)
    T = np.arange(60.0).reshape(6, 10)
    T.reshape(-1)[idx[1]] = np.inf  # a cell the sample holds
    bench.dump_map(str(tmp_path / "a"), "total_cost", T)
    a = np.load(tmp_path / "a" / "total_cost.npy")
    want = np.where(np.isinf(T), -1.0, T)  # +inf leaves as -1.0: every stored value finite
    assert a.dtype == np.float64 and np.array_equal(a, want)
    assert np.isfinite(a).all() and (a == -1.0).sum() == 1
    assert np.isinf(T).sum() == 1  # the caller's map is left as it was
    bench.dump_map(str(tmp_path / "a"), "part", T, max_bytes=160)
    b = np.load(tmp_path / "a" / "part.npy")
    assert b.dtype == np.float64 and np.array_equal(b, want.reshape(-1)[idx]) and b[1] == -1.0


def test_plain_run_turns_the_side_legs_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.sustain_s == 0 and a.cpu_sample == 0
    assert a.no_variants and a.no_parity and a.no_planner
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.sustain_s > 0 and a.cpu_sample == a.size
    assert not (a.no_variants or a.no_parity or a.no_planner)
