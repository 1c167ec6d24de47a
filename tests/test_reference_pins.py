"""The CPU oracle and the host planner against the reference planner's own code.

tests/golden/ref_*.npz were recorded by oracle/_ref/ref_driver, which is the reference's
two sources compiled unmodified (oracle/Makefile, target `ref`; tests/golden/
gen_golden_ref.py).  Nothing in them went through oracle/*.c.

(a) test_oracle_*: every recorded case through oracle_ffi -- all floating-point arrays bit
    for bit, all integer arrays, orders and return values equal.  No quantity needed the
    1 ulp allowance for a libm call: same compiler family, same libm, -ffp-contract=off on
    both sides.
(b) test_planner_*: the host planner's CPU route against the same files, directly.
(c) test_live_*: where the driver exists, fresh inputs through the reference and the oracle,
    and the driver against every committed ref_* file and every older oracle-made fixture
    that a case covers.  They skip only where neither the driver nor the reference's
    sources exist; sources without a driver is a failure (build() makes the driver).
"""
import copy
import os

import numpy as np
import pytest

import ref_cases as rc
import ref_ffi

NAMES = sorted(rc.committed_cases())
GOLD = rc.GOLD


def _family(f):
    return [n for n in NAMES if n.startswith(f + "_")]


@pytest.fixture(scope="module")
def recorded():
    return {n: rc.load_fixture(n) for n in NAMES}


def test_fixture_files_match_case_list():
    have = sorted(f[4:-4] for f in os.listdir(GOLD) if f.startswith("ref_") and f.endswith(".npz"))
    assert have == NAMES
    for n in NAMES:
        assert os.path.getsize(rc.fixture_path(n)) <= 512 * 1024, n


def test_settings_covered(recorded):
    """every family with nx > ny, nx < ny, a resolution other than 1 (the local layer
    excepted: the reference crashes there) and a non-zero offset"""
    for fam in ("setcost", "costmap", "early", "path", "local"):
        ps = [recorded[n][0]["params"] for n in _family(fam)]
        assert any(p["nx"] > p["ny"] for p in ps) and any(p["nx"] < p["ny"] for p in ps), fam
        assert any(p["offset"] != [0.0, 0.0] for p in ps), fam
        assert fam == "local" or any(p["gres"] != 1.0 for p in ps), fam


# ------------------------------------------------------------------ (a) oracle
@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference(oracle, recorded, name):
    case, want = recorded[name]
    got = rc.ORACLE[case["family"]](oracle, case)
    assert rc.differences(got, want) == []


@pytest.mark.parametrize("name", _family("setcost") + _family("path"))
def test_speed_of_recorded_fields(oracle, recorded, name):
    """ref_cases.speed_from_fields (what the GPU tests solve on) is oracle_pack_speed of the
    recorded node fields, bit for bit"""
    case, want = recorded[name]
    F = rc.speed_from_fields(want, case["params"]["gres"])
    Fo = oracle.pack_speed(want["cost"], want["hazard"], want["traff"], want["is_obstacle"],
                           res=case["params"]["gres"])
    assert F.tobytes() == Fo.tobytes() and np.isinf(F).any()


# ------------------------------------------------------------------ (b) host planner
@pytest.mark.parametrize("name", _family("setcost"))
def test_planner_set_cost_map_and_goal(dymu, recorded, name):
    case, want = recorded[name]
    got = rc.planner_setcost(dymu, case)
    assert rc.differences(got, want, keys=sorted(got)) == []
    assert {"rc_setcost", "rc_setgoal", "goal_node", "rc_goal_probes", "global_cost", "cost",
            "is_obstacle", "hazard", "traff"} <= set(got)


@pytest.mark.parametrize("name", _family("costmap"))
def test_planner_compute_cost_map(dymu, recorded, name):
    case, want = recorded[name]
    got = rc.planner_costmap(dymu, case)
    assert rc.differences(got, want, keys=sorted(got)) == []
    assert {f + s for f in ("slope", "raw_cost", "cost", "terrain", "is_obstacle", "loc_mode")
            for s in ("_1", "_2")} <= set(got)


@pytest.mark.parametrize("name", _family("path"))
def test_planner_paths_on_loaded_map(dymu, recorded, name):
    """getPath, getTotalCost and getLocomotionMode on the reference's own total-cost matrix"""
    case, want = recorded[name]
    got = rc.planner_path(dymu, case, want["total_cost"])
    assert rc.differences(got, want, keys=["path_len", "path_wp", "point_cost",
                                            "point_loc"]) == []


@pytest.mark.parametrize("name", _family("local"))
def test_planner_local_layer(dymu, recorded, name):
    case, want = recorded[name]
    got = rc.planner_local(dymu, case, want["total_cost"])
    assert rc.differences(got, want, keys=sorted(got)) == []
    assert {"trajectory", "current_path", "risk", "deviation", "hazard_matrix",
            "traff_matrix"} <= set(got)


# ------------------------------------------------------------------ (c) live
@pytest.fixture(scope="module")
def driver():
    if ref_ffi.have_driver():
        return True
    if ref_ffi.have_sources():
        pytest.fail("the reference's sources are present but oracle/_ref/ref_driver is not: "
                    "run `make -C oracle ref`")
    pytest.skip("neither the reference's sources nor the built driver exist here")


OFF = (3.5, -2.25)
SHAPES = [(44, 30, 1.0, (0.0, 0.0)), (30, 44, 0.5, OFF), (37, 26, 2.0, (1.0, 2.0))]
LOCAL_SHAPES = [(64, 40, (3.0, -2.0)), (40, 64, (0.0, 0.0)), (56, 44, (1.5, 0.5))]


def _live(oracle, case):
    want = rc.run_reference(case)
    got = rc.ORACLE[case["family"]](oracle, case)
    assert rc.differences(got, want) == []


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("seed", range(6))
def test_live_setcost(driver, oracle, shape, seed):
    _live(oracle, rc.setcost_case(*shape, seed=1000 + seed))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("seed", range(3))
def test_live_costmap(driver, oracle, shape, seed):
    n_locs, n_slopes = [(1, 5), (3, 4), (2, 1)][seed]
    _live(oracle, rc.costmap_case(*shape, seed=2000 + seed, n_locs=n_locs, n_slopes=n_slopes))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("seed", range(3))
def test_live_early(driver, oracle, shape, seed):
    _live(oracle, rc.early_case(*shape, seed=3000 + seed, constant=(seed == 2)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("seed", range(3))
def test_live_path(driver, oracle, shape, seed):
    _live(oracle, rc.path_case(*shape, seed=4000 + seed, n_locs=1 + seed % 2))


@pytest.mark.parametrize("shape", LOCAL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("approach", [0, 1], ids=["conservative", "sweeping"])
def test_live_local(driver, oracle, shape, approach):
    nx, ny, off = shape
    _live(oracle, rc.local_case(nx, ny, off, seed=5000 + 2 * approach, approach=approach))


@pytest.mark.parametrize("name", NAMES)
def test_live_driver_reproduces_fixture(driver, recorded, name):
    """the committed file's outputs are what the driver writes for the committed inputs,
    byte for byte: a fixture cannot have come from the oracle"""
    case, want = recorded[name]
    got = rc.run_reference(copy.deepcopy(case))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npy"), allow_pickle=False)


def _m1(T):
    return np.where(np.isinf(T), -1.0, T)


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _square(N, gres=1.0, lres=0.5, **kw):
    return dict(nx=N, ny=N, gres=gres, lres=lres, offset=[0.0, 0.0], **rc.PLANNER, **kw)


def test_live_older_setcost_and_early64(driver):
    """setcost64_* and early64_* (gen_golden.py, oracle-made) against the reference"""
    cost = _gold("setcost64_cost")
    g = [float(x) for x in _gold("setcost64_goal")]
    p = _square(64, goal=g + [0.0])
    r = rc.run_reference({"family": "setcost", "params": p,
                          "arrays": {"cost": cost, "goal_probes": np.array([g])}})
    assert _same(r["total_cost"], _m1(_gold("setcost64_T")))
    p = _square(64, goal=g, start=[12.0, 50.0], goal2=g, start2=[12.0, 50.0])
    r = rc.run_reference({"family": "early", "params": p, "arrays": {"cost": cost}})
    for sfx in ("_1", "_2"):
        assert r["rc" + sfx][0] == _gold("early64_rc")[0]
        assert _same(r["total_cost" + sfx], _m1(_gold("early64_T")))
        assert np.array_equal(r["closed" + sfx], _gold("early64_closed"))


def test_live_older_early256(driver):
    gi, gj, si, sj = (float(x) for x in _gold("early256_goal_start"))
    p = _square(256, goal=[gi, gj], start=[si, sj], goal2=[gi, gj], start2=[si, sj])
    r = rc.run_reference({"family": "early", "params": p,
                          "arrays": {"cost": _gold("early256_cost")}})
    assert r["rc_1"][0] == _gold("early256_rc")[0]
    assert _same(r["total_cost_1"], _m1(_gold("early256_T")))
    assert np.array_equal(r["closed_1"], _gold("early256_closed"))


def test_live_older_terrain128(driver):
    from gen_golden import terrain_inputs
    elev, terr, lut, slopes = terrain_inputs(128)
    assert _same(elev, _gold("terrain128_elev")) and _same(terr, _gold("terrain128_terrain"))
    g = [0.5 * float(x) for x in _gold("terrain128_goal")]
    p = _square(128, gres=0.5, lres=0.125, n_locs=1, goal=g + [0.0])
    arrays = dict(lut=lut, slopes=slopes, elevation=elev, terrain=terr,
                  starts=np.array([[10.0, 10.0, 0.0]]), points=np.array([[10.0, 10.0]]))
    r = rc.run_reference({"family": "path", "params": p, "arrays": arrays})
    assert _same(r["cost"], _gold("terrain128_cost"))
    assert _same(r["total_cost"], _m1(_gold("terrain128_T")))


@pytest.mark.parametrize("name,approach", [("cons", 0), ("sweep", 1)])
def test_live_older_local(driver, name, approach):
    """local_cons_* / local_sweep_* (gen_golden_local.py, oracle-made)"""
    r = rc.run_reference(rc.golden_local_case(approach))
    old = {k: _gold(f"local_{name}_{k}") for k in ("path", "traj", "hazard", "traff", "risk",
                                                   "dev", "rep")}
    assert _same(r["path"], old["path"]) and _same(r["trajectory"], old["traj"])
    assert _same(r["hazard_matrix"], old["hazard"]) and _same(r["traff_matrix"], old["traff"])
    assert _same(r["risk"], old["risk"]) and _same(r["deviation"], old["dev"])
    assert [int(r["rc_local"][0]), int(r["reconnecting_index"][0])] == old["rep"].tolist()
