"""Case inputs for the reference pins, and the same cases run through the reference
driver (ref_ffi), the oracle (oracle_ffi) and the host planner, each returning a dict
with the driver's output names so that the tests compare dict against dict.

A case is {"family", "params" (scalars and short vectors), "arrays"}.  Inputs are
synthetic and drawn from numpy's default_rng(seed): the committed fixtures store them, so
no test depends on the generator's stream.
"""
import io
import os
import zipfile

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLANNER = dict(risk_distance=1.0, reconnect_distance=1.5, risk_ratio=5.0)


def _grid(nx, ny, gres, lres, offset, **kw):
    p = dict(nx=nx, ny=ny, gres=gres, lres=lres, offset=list(offset), **PLANNER)
    p.update(kw)
    return p


def _world(p, i, j):
    """world coordinates of the (possibly fractional) node position (i, j)"""
    return [p["offset"][0] + p["gres"] * i, p["offset"][1] + p["gres"] * j]


def _free_node(rng, free, margin=3):
    """an interior node whose 3x3 neighbourhood is free"""
    ny, nx = free.shape
    for _ in range(10000):
        i, j = int(rng.integers(margin, nx - margin)), int(rng.integers(margin, ny - margin))
        if free[j - 1:j + 2, i - 1:i + 2].all():
            return i, j
    raise RuntimeError("no free node")


# ----------------------------------------------------------------------------- inputs
def random_cost(rng, nx, ny, obst_frac):
    cost = rng.uniform(1.0, 5.0, (ny, nx))
    u = rng.uniform(0.0, 1.0, (ny, nx))
    cost[u < obst_frac] = -1.0
    cost[(u >= obst_frac) & (u < 1.2 * obst_frac)] = 0.0  # cost <= 0: zero is an obstacle too
    return cost


def setcost_case(nx, ny, gres=1.0, offset=(0.0, 0.0), seed=0):
    rng = np.random.default_rng(seed)
    p = _grid(nx, ny, gres, gres / 2, offset)
    cost = random_cost(rng, nx, ny, 0.05)
    free = cost > 0
    gi, gj = _free_node(rng, free)
    p["goal"] = _world(p, gi + 0.3, gj - 0.2) + [0.7]
    # probes: an interior obstacle, the node right of it and the one above it, off the grid
    # on every side, a border node, a rounding boundary, and a valid node
    oj, oi = [c for c in np.argwhere(~free) if 2 <= c[0] < ny - 2 and 2 <= c[1] < nx - 2][0]
    vi, vj = _free_node(rng, free)
    probes = [_world(p, oi, oj), _world(p, oi + 1, oj), _world(p, oi, oj - 1),
              _world(p, -0.25, 3), _world(p, 3, -0.01), _world(p, nx - 0.4, 3),
              _world(p, 3, ny + 2), _world(p, 0.2, 5), _world(p, 5, ny - 1), _world(p, nx - 1, 5),
              _world(p, vi + 0.5, vj + 0.5), _world(p, vi - 0.49, vj + 0.49), _world(p, vi, vj)]
    return {"family": "setcost", "params": p,
            "arrays": {"cost": cost, "goal_probes": np.array(probes)}}


def terrain_arrays(rng, nx, ny, gres, n_terr, n_locs, n_slopes):
    """elevation (mostly below the last slope, some cells above it), terrain ids 0..n_terr-1
    (0 = obstacle, rare; the last id is the LUT's last row), LUT and slope range"""
    j, i = np.mgrid[0:ny, 0:nx].astype(np.float64)
    amp = 1.6 * gres
    elev = amp * np.sin(0.21 * i + rng.uniform(0, 6)) * np.cos(0.17 * j + rng.uniform(0, 6))
    elev += 0.02 * gres * i + 0.05 * gres * rng.uniform(-1, 1, (ny, nx))
    bi, bj = int(rng.integers(6, nx - 6)), int(rng.integers(6, ny - 6))
    elev[bj:bj + 2, bi:bi + 3] += 3.0 * gres  # a step steeper than the last slope value
    terr = 1.0 + ((i.astype(np.int64) // 7 + j.astype(np.int64) // 5) % (n_terr - 1))
    u = rng.uniform(0, 1, (ny, nx))
    terr[u < 0.02] = 0.0
    ci, cj = int(rng.integers(6, nx - 8)), int(rng.integers(6, ny - 8))
    terr[cj:cj + 2, ci:ci + 2] = 0.0  # a 2x2 obstacle block (has +inf neighbours: Q5)
    slopes = np.linspace(0.0, 20.0, n_slopes) if n_slopes > 1 else np.array([0.0])
    lut = rng.uniform(1.0, 6.0, n_terr * n_locs * n_slopes)
    lut = np.sort(lut.reshape(n_terr, n_locs, n_slopes), axis=2).ravel()  # cost grows with slope
    lut[:n_locs * n_slopes] = 100.0
    return dict(lut=lut, slopes=slopes, elevation=elev, terrain=terr)


def costmap_case(nx, ny, gres=1.0, offset=(0.0, 0.0), seed=0, n_locs=1, n_slopes=5, n_terr=4):
    rng = np.random.default_rng(seed)
    p = _grid(nx, ny, gres, gres / 2, offset, n_locs=n_locs)
    return {"family": "costmap", "params": p,
            "arrays": terrain_arrays(rng, nx, ny, gres, n_terr, n_locs, n_slopes)}


def early_case(nx, ny, gres=1.0, offset=(0.0, 0.0), seed=0, constant=False):
    rng = np.random.default_rng(seed)
    p = _grid(nx, ny, gres, gres / 2, offset)
    cost = np.ones((ny, nx)) if constant else random_cost(rng, nx, ny, 0.03)
    free = cost > 0
    for k in ("goal", "start", "goal2", "start2"):
        i, j = _free_node(rng, free)
        p[k] = _world(p, i + rng.uniform(-0.4, 0.4), j + rng.uniform(-0.4, 0.4))
    return {"family": "early", "params": p, "arrays": {"cost": cost}}


def _ref_obstacles(arrays, nx, ny):
    """cells computeCostMap certainly makes obstacles: terrain 0 and the border"""
    ob = arrays["terrain"] == 0
    ob[0, :] = ob[-1, :] = ob[:, 0] = ob[:, -1] = True
    return ob


def path_case(nx, ny, gres=1.0, offset=(0.0, 0.0), seed=0, n_locs=1, n_slopes=5):
    rng = np.random.default_rng(seed)
    p = _grid(nx, ny, gres, gres / 2, offset, n_locs=n_locs)
    arrays = terrain_arrays(rng, nx, ny, gres, 4, n_locs, n_slopes)
    # a wall two nodes thick with a gap one node wide: a descent through the gap crosses
    # cells that have an obstacle corner with a +inf neighbour, the NaN rule (Q5) mid-path
    t0 = arrays["terrain"] == 0
    bj, bi = np.argwhere(t0[:-1, :-1] & t0[:-1, 1:] & t0[1:, :-1] & t0[1:, 1:])[0]  # the block
    W = int(0.55 * nx)
    arrays["terrain"][:, W:W + 2] = 0.0
    arrays["terrain"][ny // 2, W:W + 2] = 1.0
    ob = _ref_obstacles(arrays, nx, ny)
    free = ~ob
    right = free.copy()
    right[:, :W + 4] = False
    left = free.copy()
    left[:, W - 2:] = False
    gi, gj = _free_node(rng, right, margin=4)
    p["goal"] = _world(p, gi, gj) + [0.4]
    starts = []
    for side in (right, right, left, left):
        i, j = _free_node(rng, side, margin=4)
        starts.append(_world(p, i + rng.uniform(0, 0.9), j + rng.uniform(0, 0.9)) + [0.3])
    starts.append(_world(p, gi + 0.6, gj - 0.7) + [0.0])  # next to the goal
    # cells around interior obstacles: the descent's first gradient meets +inf there (Q5)
    inner = [c for c in np.argwhere(arrays["terrain"] == 0)
             if 3 <= c[0] < ny - 3 and 3 <= c[1] < nx - 3]
    for (oj, oi) in inner[:4]:
        starts.append(_world(p, oi - 1.4, oj + 0.3) + [0.0])
        starts.append(_world(p, oi + 1.2, oj - 1.6) + [0.0])
    for (di, dj) in ((-0.5, 0.5), (-1.6, 0.4), (2.6, 0.6), (0.5, -1.6), (0.5, 2.7), (-2.3, -2.2),
                     (3.4, 3.3), (-2.5, 1.0), (1.0, 4.2), (4.3, 0.5), (0.6, -3.1)):
        starts.append(_world(p, bi + di, bj + dj) + [0.0])
    pts = [_world(p, rng.uniform(1, nx - 2), rng.uniform(1, ny - 2)) for _ in range(12)]
    pts += [_world(p, rng.uniform(1, nx - 2), ny - 1 + 0.3)]      # the last row
    pts += [_world(p, nx - 2 + 0.6, rng.uniform(1, ny - 2))]      # the last whole cell column
    for (oj, oi) in inner[:3]:
        pts += [_world(p, oi - 0.7, oj + 0.2), _world(p, oi + 0.3, oj + 0.4)]
    pts += [_world(p, gi, gj), _world(p, 3, 4)]                   # on nodes
    arrays["starts"] = np.array(starts)
    arrays["points"] = np.array(pts)
    return {"family": "path", "params": p, "arrays": arrays}


def disc_image(rover, centre, radius, res, size):
    """size x size image at res m/pixel centred on rover (row j at
    y = rover_y + res*size/2 - j*res), a disc of value 1"""
    img = np.zeros((size, size), dtype=np.uint8)
    ox = rover[0] - res * size / 2
    oy = rover[1] + res * size / 2
    j, i = np.mgrid[0:size, 0:size]
    img[(ox + i * res - centre[0]) ** 2 + (oy - j * res - centre[1]) ** 2 <= radius ** 2] = 1
    return img


def golden_local_case(approach):
    """the scene of gen_golden_local.py (48^2 terrain, goal (36, 32), start (7.3, 9.1))"""
    from gen_golden import terrain_inputs
    N = 48
    elev, terr, lut, slopes = terrain_inputs(N)
    p = _grid(N, N, 1.0, 0.25, (0.0, 0.0), n_locs=1, approach=approach)
    p["goal"] = [36.0, 32.0, 0.3]
    p["start"] = [7.3, 9.1, 0.0]
    p["scene"] = [2, 10, 0.8, 36]  # rover waypoint, disc centre waypoint, radius, image size
    return {"family": "local", "params": p,
            "arrays": dict(lut=lut, slopes=slopes, elevation=elev, terrain=terr)}


def local_case(nx, ny, offset=(0.0, 0.0), seed=0, approach=0, lres=0.25):
    rng = np.random.default_rng(seed)
    p = _grid(nx, ny, 1.0, lres, offset, n_locs=1, approach=approach)
    j, i = np.mgrid[0:ny, 0:nx].astype(np.float64)
    elev = 1.2 * np.sin(0.11 * i + rng.uniform(0, 6)) * np.cos(0.13 * j) + 0.01 * j
    terr = 1.0 + ((i.astype(np.int64) // 9 + j.astype(np.int64) // 6) % 2)
    lut = np.array([100.0] * 5 + [1, 1.5, 2, 3, 5] + [2, 2.5, 3, 4, 6], dtype=np.float64)
    slopes = np.array([0.0, 5.0, 10.0, 15.0, 20.0])
    gi, gj = int(0.75 * nx), int(0.7 * ny)
    p["goal"] = _world(p, gi, gj) + [0.3]
    p["start"] = _world(p, 6 + rng.uniform(0, 1), 7 + rng.uniform(0, 1)) + [0.0]
    p["scene"] = [2, 10, 0.8, 36]
    return {"family": "local", "params": p,
            "arrays": dict(lut=lut, slopes=slopes, elevation=elev, terrain=terr)}


def local_scene(case, path):
    """rover position, image and its resolution for a local case, from the global path
    (x, y, z, heading rows, world coordinates) the first stage produced"""
    p = case["params"]
    ri, ci, radius, size = p["scene"]
    rover = tuple(path[int(ri)][:2])
    centre = tuple(path[int(ci)][:2])
    img = disc_image(rover, centre, radius, p["lres"], int(size))
    return rover, img, p["lres"]


# ----------------------------------------------------------------------------- reference
def run_reference(case):
    import ref_ffi
    params = {k: v for k, v in case["params"].items() if k != "scene"}
    arrays = dict(case["arrays"])
    if case["family"] != "local":
        return ref_ffi.run(case["family"], params, arrays)
    if "image" not in arrays:  # stage 1: the global path places the rover and the obstacle
        first = ref_ffi.run("local", params, arrays)
        rover, img, res = local_scene(case, first["path"])
        case["arrays"]["image"] = img
        case["params"]["rover"] = list(rover)
        case["params"]["image_res"] = res
        params = {k: v for k, v in case["params"].items() if k != "scene"}
        arrays = dict(case["arrays"])
    img = arrays["image"]
    params["image_size"] = [img.shape[1], img.shape[0], img.shape[2] if img.ndim == 3 else 1]
    return ref_ffi.run("local", params, arrays)


# ----------------------------------------------------------------------------- oracle
def _minus1(T):
    return np.where(np.isinf(T), -1.0, T)


def _oracle_setcost_state(o, cost):
    ny, nx = cost.shape
    st = o.new_state(nx, ny)
    o.lib.oracle_set_cost_map(np.ascontiguousarray(cost).ravel(), cost.size, st["cost"].ravel(),
                              st["is_obstacle"].ravel(), st["traff"].ravel(),
                              st["hazard"].ravel())
    return st


def _speed(o, st, res):
    return o.pack_speed(st["cost"], st["hazard"], st["traff"], st["is_obstacle"], res=res)


def _global_cost(st):
    return np.where(st["is_obstacle"] != 0, -1.0, st["cost"] * (2 + st["hazard"] - st["traff"]))


def _node(o, p, w, obst):
    return o.set_goal(p["nx"], p["ny"], p["gres"], p["offset"], w, obst)


def oracle_setcost(o, case):
    p, cost = case["params"], case["arrays"]["cost"]
    st = _oracle_setcost_state(o, cost)
    out = {"rc_setcost_wrong_shape": 0, "rc_setcost": 1, "rc_solve_no_goal": 0}
    rows = []
    for w in case["arrays"]["goal_probes"]:
        g = _node(o, p, w, st["is_obstacle"])
        rows.append([1, g[0], g[1]] if g else [0, -1, -1])
    out["rc_goal_probes"] = np.array(rows, dtype=np.int64)
    g = _node(o, p, p["goal"], st["is_obstacle"])
    out["rc_setgoal"] = int(g is not None)
    out["goal_node"] = np.array(g if g else (-1, -1), dtype=np.int64)
    T, _ = o.fmm(_speed(o, st, p["gres"]), g, linear=True)
    out["rc_solve"] = 1
    out["total_cost"] = _minus1(T)
    out["global_cost"] = _global_cost(st)
    out["hazard_matrix"] = out["hazard"] = st["hazard"]
    out["traff_matrix"] = out["traff"] = st["traff"]
    out["cost"] = st["cost"]
    out["is_obstacle"] = st["is_obstacle"].astype(np.int64)
    return out


def _oracle_costmap_once(o, st, case):
    p, a = case["params"], case["arrays"]
    o.compute_cost_map(st, p["gres"], a["lut"], a["slopes"], int(p["n_locs"]), a["elevation"],
                       a["terrain"])


def _costmap_fields(st, sfx):
    return {"is_obstacle" + sfx: st["is_obstacle"].astype(np.int64), "cost" + sfx: st["cost"].copy(),
            "hazard" + sfx: st["hazard"].copy(), "traff" + sfx: st["traff"].copy(),
            "slope" + sfx: st["slope"].copy(), "raw_cost" + sfx: st["raw_cost"].copy(),
            "terrain" + sfx: st["terrain"].astype(np.int64),
            "loc_mode" + sfx: st["loc_mode"].astype(np.int64)}


def oracle_costmap(o, case):
    p = case["params"]
    st = o.new_state(p["nx"], p["ny"])
    out = {}
    for sfx in ("_1", "_2"):
        _oracle_costmap_once(o, st, case)
        out["rc" + sfx] = 1
        out.update(_costmap_fields(st, sfx))
    return out


def _band_lists(T, closed, seq):
    """(narrowband, propagated) as (i, j) rows in the reference's stored order"""
    reached = np.isfinite(T)
    rj, ri = np.nonzero(reached)
    order = np.argsort(seq[rj, ri], kind="stable")
    prop = np.stack([ri, rj], 1)[order].astype(np.int64)
    inband = (closed[prop[:, 1], prop[:, 0]] == 0)
    return prop[inband], prop


def _next_min(T, band):
    if len(band) == 0:
        return np.array([-1, -1], dtype=np.int64)
    v = T[band[:, 1], band[:, 0]]
    return band[int(np.argmin(v))]  # first strict minimum in band order


def oracle_early(o, case):
    p, cost = case["params"], case["arrays"]["cost"]
    st = _oracle_setcost_state(o, cost)
    F = _speed(o, st, p["gres"])
    out = {}
    for sfx, gk, sk in (("_1", "goal", "start"), ("_2", "goal2", "start2")):
        g = _node(o, p, p[gk], st["is_obstacle"])
        out["rc_setgoal" + sfx] = int(g is not None)
        x = (p[sk][0] - p["offset"][0]) / p["gres"] + 0.5
        y = (p[sk][1] - p["offset"][1]) / p["gres"] + 0.5
        s = (int(x), int(y))
        T, rc, closed, seq = o.fmm_order(F, g, start=s)
        Tl, rcl, closedl = o.fmm(F, g, start=s, linear=True, want_closed=True)
        assert rc == rcl and np.array_equal(T, Tl) and np.array_equal(closed, closedl)
        out["rc" + sfx] = rc
        out["total_cost" + sfx] = _minus1(T)
        out["closed" + sfx] = closed.astype(np.int64)
        band, prop = _band_lists(T, closed, seq)
        out["narrowband" + sfx] = band
        out["propagated" + sfx] = prop
        out["next_min" + sfx] = _next_min(T, band)
    out["total_cost_reset"] = np.full_like(cost, -1.0)
    out["propagated_after_reset"] = 0
    return out


def _oracle_terrain_layer(o, case):
    p = case["params"]
    st = o.new_state(p["nx"], p["ny"])
    _oracle_costmap_once(o, st, case)
    g = _node(o, p, p["goal"], st["is_obstacle"])
    T, _ = o.fmm(_speed(o, st, p["gres"]), g, linear=True)
    return st, g, T


def _oracle_local_ctx(o, case, st, g, T):
    p = case["params"]
    L = o.local(p["nx"], p["ny"], p["gres"], p["lres"], offset=tuple(p["offset"]),
                risk_distance=p["risk_distance"], reconnect_distance=p["reconnect_distance"],
                risk_ratio=p["risk_ratio"], approach=int(p.get("approach", 0)))
    L.set_global(st["is_obstacle"], T, g, goal_heading=p["goal"][2],
                 elev=case["arrays"]["elevation"], hazard=st["hazard"], traff=st["traff"])
    return L


def oracle_path(o, case):
    p, a = case["params"], case["arrays"]
    st, g, T = _oracle_terrain_layer(o, case)
    out = {"rc_setgoal": int(g is not None), "rc_solve": 1, "total_cost": _minus1(T)}
    out.update(_costmap_fields(st, ""))
    L = _oracle_local_ctx(o, case, st, g, T)
    lens, wps = [], []
    for s in a["starts"]:
        _, path = L.get_path((s[0], s[1], 0.0, s[2]))
        lens.append(len(path))
        wps.append(path)
    out["path_len"] = np.array(lens, dtype=np.int64)
    out["path_wp"] = np.concatenate(wps, axis=0).reshape(-1, 4)
    out["point_cost"] = np.array([L.total_cost(x, y) for x, y in a["points"]])
    loc = []
    for x, y in a["points"]:
        i = int((x - p["offset"][0]) / p["gres"] + 0.5)
        j = int((y - p["offset"][1]) / p["gres"] + 0.5)
        loc.append(st["loc_mode"][j, i])
    out["point_loc"] = np.array(loc, dtype=np.int64)
    return out


def oracle_local(o, case):
    p, a = case["params"], case["arrays"]
    st, g, T = _oracle_terrain_layer(o, case)
    out = {"rc_setgoal": int(g is not None), "rc_solve": 1, "total_cost": _minus1(T)}
    L = _oracle_local_ctx(o, case, st, g, T)
    s = p["start"]
    _, out["path"] = L.get_path((s[0], s[1], 0.0, s[2]))
    rover = tuple(p["rover"])
    rep, traj = L.local_planning(rover, a["image"], p["image_res"])
    out["rc_local"] = int(rep)
    out["trajectory"] = traj.reshape(-1, 4)
    out["current_path"] = L.path.reshape(-1, 4)
    out["reconnecting_index"] = L.reconnecting_index()
    out["risk"] = L.risk_matrix(*rover)
    out["deviation"] = L.deviation_matrix(*rover)
    hd, tr = L.hazard_traff()
    out["hazard_matrix"], out["traff_matrix"] = hd, tr
    st2 = dict(st, hazard=hd, traff=tr)
    out["global_cost"] = _global_cost(st2)
    T2, _ = o.fmm(_speed(o, st2, p["gres"]), g, linear=True)
    out["rc_resolve"] = 1
    out["total_cost_2"] = _minus1(T2)
    return out


ORACLE = {"setcost": oracle_setcost, "costmap": oracle_costmap, "early": oracle_early,
          "path": oracle_path, "local": oracle_local}


def speed_from_fields(fields, gres):
    """the reference's C = global_res * cost * (2 + hazard_density - trafficability)
    (:527-528) of recorded node fields, +inf on obstacles; numpy rounds each operation as
    the reference's build does"""
    F = gres * fields["cost"] * (2 + fields["hazard"] - fields["traff"])
    return np.where(np.asarray(fields["is_obstacle"]) != 0, np.inf, F)


# ----------------------------------------------------------------------------- compare
def differences(got, want, keys=None):
    """names whose arrays are not bit-identical (shape, then bytes of the float64 / int64
    image; NaN compares by its bits)"""
    bad = []
    for k in (keys if keys is not None else sorted(want)):
        if k not in got:
            bad.append(k + " (missing)")
            continue
        w = np.asarray(want[k])
        g = np.asarray(got[k])
        dt = np.float64 if w.dtype.kind == "f" else np.int64
        w = np.atleast_1d(w).astype(dt)
        g = np.atleast_1d(g).astype(dt)
        if w.shape != g.shape and w.size == g.size == 0:
            continue
        if w.shape != g.shape or w.tobytes() != g.tobytes():
            bad.append(k)
    return bad


# ----------------------------------------------------------------------------- host planner
def _inf(M):
    return np.where(M == -1.0, np.inf, M)


def _new_planner(dymu, p):
    pl = dymu.Planner(risk_distance=p["risk_distance"],
                      reconnect_distance=p["reconnect_distance"], risk_ratio=p["risk_ratio"],
                      approach=int(p.get("approach", 0)))
    assert pl.initGlobalLayer(p["gres"], p["lres"], p["nx"], p["ny"], offset=tuple(p["offset"]))
    return pl


def _mode_names(p):
    return [f"mode{k}" for k in range(int(p["n_locs"]))]


def _planner_nodes(pl, p, sfx, cost_fields):
    nx, ny = p["nx"], p["ny"]
    names = ["is_obstacle", "cost", "hazard_density", "trafficability"]
    if cost_fields:
        names += ["slope", "raw_cost", "terrain"]
    cols = {k: [] for k in names}
    for j in range(ny):
        for i in range(nx):
            n = pl.getGlobalNode(i, j)
            for k in names:
                cols[k].append(n[k])
    out = {}
    for k, v in cols.items():
        name = {"hazard_density": "hazard", "trafficability": "traff"}.get(k, k)
        dt = np.int64 if k in ("is_obstacle", "terrain") else np.float64
        out[name + sfx] = np.array(v, dtype=dt).reshape(ny, nx)
    if cost_fields:
        modes = _mode_names(p)
        loc = [modes.index(m) if m in modes else -1
               for m in (pl.getLocomotionMode(_world(p, i, j)) for j in range(ny)
                         for i in range(nx))]
        out["loc_mode" + sfx] = np.array(loc, dtype=np.int64).reshape(ny, nx)
    return out


def planner_setcost(dymu, case):
    """what the host planner computes of a setcost case without a device"""
    p, a = case["params"], case["arrays"]
    pl = _new_planner(dymu, p)
    out = {"rc_setcost_wrong_shape": int(pl.setCostMap(np.ones((p["ny"] + 1, p["nx"])))),
           "rc_setcost": int(pl.setCostMap(a["cost"]))}
    rows = []
    for w in a["goal_probes"]:
        q = _new_planner(dymu, p)
        q.setCostMap(a["cost"])
        ok = q.setGoal(tuple(w))
        rows.append([1, q.goalI(), q.goalJ()] if ok else [0, -1, -1])
        q.close()
    out["rc_goal_probes"] = np.array(rows, dtype=np.int64)
    g = p["goal"]
    ok = pl.setGoal((g[0], g[1], 0.0, g[2]))
    out["rc_setgoal"] = int(ok)
    out["goal_node"] = np.array([pl.goalI(), pl.goalJ()] if ok else [-1, -1], dtype=np.int64)
    out["global_cost"] = pl.getGlobalCostMatrix()
    out["hazard_matrix"] = pl.getHazardDensityMatrix()
    out["traff_matrix"] = pl.getTrafficabilityMatrix()
    out.update(_planner_nodes(pl, p, "", False))
    pl.close()
    return out


def _planner_costmap_once(pl, case):
    a = case["arrays"]
    return pl.computeCostMap(a["lut"], a["slopes"], _mode_names(case["params"]), a["elevation"],
                             a["terrain"])


def planner_costmap(dymu, case):
    p = case["params"]
    pl = _new_planner(dymu, p)
    out = {}
    for sfx in ("_1", "_2"):
        out["rc" + sfx] = int(_planner_costmap_once(pl, case))
        out.update(_planner_nodes(pl, p, sfx, True))
    pl.close()
    return out


def _planner_loaded(dymu, case, total_cost):
    """a planner with the case's cost map and goal, and the given total-cost matrix (-1 for
    unreached) installed instead of a solve"""
    p = case["params"]
    pl = _new_planner(dymu, p)
    assert _planner_costmap_once(pl, case)
    g = p["goal"]
    assert pl.setGoal((g[0], g[1], 0.0, g[2]))
    assert pl.loadTotalCostMap(_inf(total_cost))
    return pl


def planner_path(dymu, case, total_cost):
    p, a = case["params"], case["arrays"]
    pl = _planner_loaded(dymu, case, total_cost)
    out = {}
    lens, wps = [], []
    for s in a["starts"]:
        path = pl.getPath((s[0], s[1], 0.0, s[2]))
        lens.append(len(path))
        wps.append(path)
    out["path_len"] = np.array(lens, dtype=np.int64)
    out["path_wp"] = np.concatenate(wps, axis=0).reshape(-1, 4)
    out["point_cost"] = np.array([pl.getTotalCost((x, y)) for x, y in a["points"]])
    modes = _mode_names(p)
    out["point_loc"] = np.array([modes.index(m) if m in modes else -1 for m in
                                 (pl.getLocomotionMode((x, y)) for x, y in a["points"])],
                                dtype=np.int64)
    pl.close()
    return out


def planner_local(dymu, case, total_cost, keep=False):
    p, a = case["params"], case["arrays"]
    pl = _planner_loaded(dymu, case, total_cost)
    s = p["start"]
    out = {"path": pl.getPath((s[0], s[1], 0.0, s[2]))}
    rover = tuple(p["rover"])
    rep, traj, _ = pl.computeLocalPlanning(rover + (0.0, 0.0), a["image"], p["image_res"])
    out["rc_local"] = int(rep)
    out["trajectory"] = traj.reshape(-1, 4)
    out["current_path"] = pl.current_path.reshape(-1, 4)
    out["reconnecting_index"] = pl.getReconnectingIndex()
    out["risk"] = pl.getRiskMatrix(rover)
    out["deviation"] = pl.getDeviationMatrix(rover)
    out["hazard_matrix"] = pl.getHazardDensityMatrix()
    out["traff_matrix"] = pl.getTrafficabilityMatrix()
    out["global_cost"] = pl.getGlobalCostMatrix()
    if keep:
        return out, pl
    pl.close()
    return out


# ----------------------------------------------------------------------------- fixtures
def committed_cases():
    """name -> case of every tests/golden/ref_NAME.npz, as gen_golden_ref.py draws them.
    Between them every family runs with nx > ny, nx < ny, a resolution other than 1 and a
    non-zero offset -- but the local layer only at resolution 1: with any other the
    reference's own sub-cell lookup indexes outside its map (it crashes)."""
    off = (3.5, -2.25)
    return {
        "setcost_96x64": setcost_case(96, 64, seed=11),
        "setcost_64x96": setcost_case(64, 96, 0.5, off, seed=12),
        "setcost_33x47": setcost_case(33, 47, 2.0, (1.0, 2.0), seed=13),
        "costmap_96x64": costmap_case(96, 64, seed=21),
        "costmap_64x96": costmap_case(64, 96, 0.5, off, seed=22, n_locs=3),
        "costmap_40x56": costmap_case(40, 56, 2.0, (1.0, 2.0), seed=23, n_locs=2, n_slopes=1),
        "early_96x64": early_case(96, 64, seed=31),
        "early_64x96": early_case(64, 96, 0.5, off, seed=32),
        "early_48x40": early_case(48, 40, 1.0, (1.0, 2.0), seed=33, constant=True),
        "path_96x64": path_case(96, 64, seed=42),
        "path_64x96": path_case(64, 96, 0.5, off, seed=40, n_locs=2),
        "path_33x47": path_case(33, 47, 2.0, (1.0, 2.0), seed=41),
        "local_cons": golden_local_case(0),
        "local_sweep": golden_local_case(1),
        "local_64x40": local_case(64, 40, (3.0, -2.0), seed=51, approach=0),
        "local_40x64": local_case(40, 64, (1.5, 0.5), seed=52, approach=1),
    }


def fixture_path(name):
    return os.path.join(GOLD, f"ref_{name}.npz")


def save_fixture(name, case, out):
    """one .npz per case: family, p_* parameters, in_* input arrays, out_* what the
    reference produced.  Written with fixed zip timestamps, so equal content gives equal
    bytes."""
    items = {"family": np.array(case["family"])}
    for k, v in case["params"].items():
        items["p_" + k] = np.atleast_1d(np.asarray(v, dtype=np.float64))
    for k, v in case["arrays"].items():
        items["in_" + k] = np.asarray(v)
    for k, v in out.items():
        items["out_" + k] = np.asarray(v)
    with zipfile.ZipFile(fixture_path(name), "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(items):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(items[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)),
                       buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


_INT_PARAMS = ("nx", "ny", "n_locs", "approach")


def load_fixture(name):
    """(case, reference outputs) of tests/golden/ref_NAME.npz"""
    with np.load(fixture_path(name), allow_pickle=False) as z:
        case = {"family": str(np.atleast_1d(z["family"])[0]), "params": {}, "arrays": {}}
        out = {}
        for k in z.files:
            if k.startswith("p_"):
                v = z[k]
                key = k[2:]
                if key in _INT_PARAMS:
                    case["params"][key] = int(v[0])
                elif v.size == 1 and key not in ("scene",):
                    case["params"][key] = float(v[0])
                else:
                    case["params"][key] = [float(x) for x in v]
            elif k.startswith("in_"):
                case["arrays"][k[3:]] = z[k]
            elif k.startswith("out_"):
                out[k[4:]] = z[k]
    return case, out
