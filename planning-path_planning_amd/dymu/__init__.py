"""dymu -- Python binding of the MI355X DyMu total-cost propagation engine.

Thin ctypes layer over the two in-tree shared libraries:

* ``lib/libdymu_fim.so``     -- HIP kernels + C-ABI (include/dymu_fim.h)
* ``lib/libdymu_planner.so`` -- host C++ ``PathPlanning_lib::DyMuPathPlanner``
                                (include/DyMu.hpp) behind include/dymu_planner.h
* ``lib/libdymu_dist.so``    -- row-slab sharded solve over RCCL
                                (include/dymu_dist.h; binding in dymu.dist)

There is no CPU fallback: if the HIP library is missing or no device is
visible, every entry point raises ``DymuError``.  The CPU oracle under
``oracle/`` is test infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DYMU_LIBDIR: load the libraries from another directory (A/B builds)
_LIBDIR = os.environ.get("DYMU_LIBDIR") or os.path.normpath(os.path.join(_HERE, "..", "lib"))

DYMU_OK = 0
_ERRS = {
    -1: "invalid argument",
    -2: "HIP runtime error",
    -3: "device out of memory",
    -4: "pass cap reached before convergence",
    -5: "no HIP device",
    -6: "RCCL error",
    -7: "call out of sequence",
}


class DymuError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__(f"dymu status {status} ({_ERRS.get(status, 'unknown')}) {what}".strip())


class DymuOpts(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("passes_per_check", ctypes.c_int),
        ("max_passes", ctypes.c_int),
        ("max_inner", ctypes.c_int),
        ("grid_blocks", ctypes.c_int),
        ("kernel", ctypes.c_int),
        ("prio_target", ctypes.c_int),
        ("exact_sqrt", ctypes.c_int),
        ("deterministic", ctypes.c_int),
    ]


class DymuDomain(ctypes.Structure):
    _fields_ = [
        ("F", ctypes.c_void_p),
        ("T", ctypes.c_void_p),
        ("ld", ctypes.c_uint64),
        ("nx", ctypes.c_uint32),
        ("nrows", ctypes.c_uint32),
        ("ghost_lo", ctypes.c_int32),
        ("ghost_hi", ctypes.c_int32),
    ]


PEER_CTL_BYTES = 128  # DYMU_PEER_CTL_BYTES
PEER_CTL_RMIN = (32, 16)  # byte offset and size of the two rmin words (all ones at the start)


class DymuPeerLinks(ctypes.Structure):
    """dymu_peer_links: side 0 = the link to rank-1, side 1 = to rank+1; 0 = none."""
    _fields_ = [
        ("recv", ctypes.c_void_p * 2),
        ("recv_tag", ctypes.c_void_p * 2),
        ("send", ctypes.c_void_p * 2),
        ("send_tag", ctypes.c_void_p * 2),
        ("last", ctypes.c_void_p * 2),
        ("ctl", ctypes.c_void_p),
    ]


class DymuCostState(ctypes.Structure):
    """dymu_cost_state: device pointers of the planner node fields."""
    FIELDS = ("cost", "raw_cost", "slope", "terrain", "is_obstacle", "hazard", "traff",
              "loc_mode")
    _fields_ = [(f, ctypes.c_void_p) for f in FIELDS]


class DymuRegion(ctypes.Structure):
    _fields_ = [("i0", ctypes.c_uint32), ("j0", ctypes.c_uint32), ("i1", ctypes.c_uint32),
                ("j1", ctypes.c_uint32), ("n_range", ctypes.c_uint64), ("r_const", ctypes.c_double)]


class DymuReduceSummary(ctypes.Structure):
    """dymu_reduce_summary (include/dymu_fim.h)."""
    _fields_ = [("min_value", ctypes.c_double), ("min_i", ctypes.c_uint32),
                ("min_j", ctypes.c_uint32), ("min_plane", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("n_finite", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {"min_value": self.min_value, "min_i": self.min_i, "min_j": self.min_j,
                "min_plane": self.min_plane, "n_finite": self.n_finite}


class DymuRouteOut(ctypes.Structure):
    """dymu_route_out (include/dymu_fim.h): output maps, NULL = not computed."""
    _fields_ = [("sink", ctypes.c_void_p), ("axis", ctypes.c_void_p), ("diag", ctypes.c_void_p),
                ("length", ctypes.c_void_p), ("integral", ctypes.c_void_p * 4),
                ("vmin", ctypes.c_void_p * 4), ("vmax", ctypes.c_void_p * 4),
                ("ld", ctypes.c_uint64)]


ROUTE_OUTPUTS = ("sink", "axis", "diag", "length", "integral", "vmin", "vmax")


class DymuUsageOut(ctypes.Structure):
    """dymu_usage_out (include/dymu_fim.h): output maps, NULL = not computed."""
    _fields_ = [("usage", ctypes.c_void_p), ("far", ctypes.c_void_p), ("sink", ctypes.c_void_p),
                ("ld", ctypes.c_uint64)]


USAGE_OUTPUTS = ("usage", "far", "sink", "catchment")


class DymuCorridorInfo(ctypes.Structure):
    """dymu_corridor_info (include/dymu_planner.h)."""
    _fields_ = [("d_min", ctypes.c_double), ("min_i", ctypes.c_uint32), ("min_j", ctypes.c_uint32),
                ("count", ctypes.c_uint64), ("i0", ctypes.c_uint32), ("j0", ctypes.c_uint32),
                ("i1", ctypes.c_uint32), ("j1", ctypes.c_uint32), ("bound", ctypes.c_double)]


REDUCE_SUM, REDUCE_MAX, REDUCE_MIN = 0, 1, 2
_REDUCE_OPS = {"sum": REDUCE_SUM, "max": REDUCE_MAX, "min": REDUCE_MIN}


def _reduce_op(op) -> int:
    return _REDUCE_OPS[op.lower()] if isinstance(op, str) else int(op)


class DymuStats(ctypes.Structure):
    _fields_ = [
        ("passes", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("tile_visits", ctypes.c_uint64),
        ("inner_sweeps", ctypes.c_uint64),
        ("max_active", ctypes.c_uint64),
        ("rounds", ctypes.c_uint64),
        ("ms", ctypes.c_double),
        ("tile_w", ctypes.c_int),
        ("tile_h", ctypes.c_int),
        ("kernel", ctypes.c_int),
        ("reserved", ctypes.c_int),
        ("deferred", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_u32, _u64, _i32, _vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p


class DymuDomState(ctypes.Structure):
    """dymu_dom_state (include/dymu_fim.h): scalars out, host buffers in."""
    _fields_ = [
        ("eb", _u32), ("ntiles", _u32), ("tiles_cap", _u32), ("variant", ctypes.c_int32),
        ("p", _u64), ("F", _vp), ("T", _vp), ("ld", _u64), ("nx", _u32), ("ny", _u32),
        ("has_keys", ctypes.c_int32), ("has_ec", ctypes.c_int32), ("list_n", _u64),
        ("minkey", _u64 * 3), ("base", ctypes.c_double * 3), ("delta", ctypes.c_double),
        ("tile_epoch", _vp), ("tile_epoch_cap", _u64), ("counts", _vp), ("list_raw", _vp),
        ("list_tile", _vp), ("list_cap", _u64), ("keys", _vp), ("keys_cap", _u64),
        ("hist", _vp), ("ec", _vp), ("ec_cap", _u64),
    ]

# name -> (restype, argtypes)
# dymu_seed (include/dymu_fim.h): a source cell and its start value
SEED_DTYPE = np.dtype([("i", np.uint32), ("j", np.uint32), ("t0", np.float64)], align=True)
LABEL_NONE = 0xFFFFFFFF
# dymu_batch_seed: a seed of plane `plane` of a batch
BATCH_SEED_DTYPE = np.dtype([("plane", np.uint32), ("i", np.uint32), ("j", np.uint32),
                             ("reserved", np.uint32), ("t0", np.float64)], align=True)
# dymu_batch_window: a changed window of plane `plane` of a batch
BATCH_WINDOW_DTYPE = np.dtype([("plane", np.uint32), ("i0", np.uint32), ("j0", np.uint32),
                               ("w", np.uint32), ("h", np.uint32), ("reserved", np.uint32)],
                              align=True)
# dymu_cell / dymu_batch_cell: the target cells of the early-exit solves
CELL_DTYPE = np.dtype([("i", np.uint32), ("j", np.uint32)], align=True)
BATCH_CELL_DTYPE = np.dtype([("plane", np.uint32), ("i", np.uint32), ("j", np.uint32),
                             ("reserved", np.uint32)], align=True)
# dymu_path_stat: the record of one path (include/dymu_fim.h)
PATH_FIELDS = 4
PATH_STAT_DTYPE = np.dtype([("status", np.int32), ("sink", np.int32), ("count", np.uint32),
                            ("reserved", np.uint32), ("length", np.float64),
                            ("last_hop", np.float64), ("integral", np.float64, (PATH_FIELDS,)),
                            ("vmin", np.float64, (PATH_FIELDS,)),
                            ("vmax", np.float64, (PATH_FIELDS,)),
                            ("skipped", np.uint32, (PATH_FIELDS,))], align=True)
# dymu_arrive_stat: the record of one arriving path (include/dymu_fim.h)
ARRIVE_STAT_DTYPE = np.dtype([("status", np.int32), ("sink", np.int32), ("count", np.uint32),
                              ("hops", np.uint32), ("length", np.float64),
                              ("start_cost", np.float64)], align=True)

FIM_SYMBOLS = {
    "dymu_create": (_i32, [ctypes.POINTER(_vp), ctypes.POINTER(DymuOpts)]),
    "dymu_destroy": (_i32, [_vp]),
    "dymu_solve": (_i32, [_vp, _dp, _u32, _u32, _u32, _u32, _dp, ctypes.POINTER(DymuStats)]),
    "dymu_solve_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _u32, _u32, _vp,
                                 ctypes.POINTER(DymuStats)]),
    "dymu_synth_speed": (_i32, [_vp, _vp, _u32, _u32, _u64, _u64, _u64, ctypes.c_double, _u64,
                                _u32, _u32, _vp]),
    "dymu_device_alloc": (_i32, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "dymu_device_free": (_i32, [_vp, _vp]),
    "dymu_memcpy_d2h": (_i32, [_vp, _vp, _vp, ctypes.c_size_t]),
    "dymu_memcpy_h2d": (_i32, [_vp, _vp, _vp, ctypes.c_size_t]),
    "dymu_set_profiling": (_i32, [_vp, _i32]),
    "dymu_set_pass_stats": (_i32, [_vp, _i32]),
    "dymu_last_update_stats": (_i32, [_vp, ctypes.POINTER(_u64)]),
    "dymu_last_pass_stats": (_i32, [_vp, _vp, _u64, ctypes.POINTER(_u64)]),
    "dymu_eikonal_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _i32]),
    "dymu_pass_scan_probe": (_i32, [_vp, _vp, _vp, _u32, ctypes.c_float, ctypes.c_float, _vp,
                                    ctypes.POINTER(ctypes.c_int32)]),
    "dymu_slab_rows": (_i32, [_u32, _u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "dymu_dom_begin": (_i32, [_vp, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, _vp]),
    "dymu_dom_run": (_i32, [_vp, _u32, _vp]),
    "dymu_dom_merge_ghosts": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "dymu_dom_pending": (_i32, [_vp, _vp, ctypes.POINTER(_u64)]),
    "dymu_dom_exchange": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "dymu_dom_round_supported": (_i32, [_vp, _u32]),
    "dymu_dom_round_capable": (_i32, [_vp, _u32, _u32, _u32]),
    "dymu_dom_round": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "dymu_dom_round_peer": (_i32, [_vp, _u32, _vp, _vp]),
    "dymu_count_equal": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double,
                                ctypes.POINTER(_u64), _vp]),
    "dymu_find_equal": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double, _vp, _u64,
                               ctypes.POINTER(_u64), _vp]),
    "dymu_dom_post_status": (_i32, [_vp, _vp, _vp, _u32]),
    "dymu_dom_post": (_i32, [_vp, _vp, ctypes.POINTER(_u32)]),
    "dymu_dom_wait_post": (_i32, [_vp, _u32, ctypes.c_double, ctypes.POINTER(ctypes.c_int32),
                                  _vp]),
    "dymu_set_stepping": (_i32, [_vp, _i32]),
    "dymu_dom_min_key": (_i32, [_vp, _vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_dom_snapshot": (_i32, [_vp, _vp, _vp]),
    "dymu_debug_raise_epoch_base": (_i32, [_vp, _u32]),
    "dymu_dom_finish": (_i32, [_vp, _vp, ctypes.POINTER(DymuStats)]),
    "dymu_last_pass_timing": (_i32, [_vp, ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_uint64)]),
    "dymu_compute_cost_map": (_i32, [_vp, _u32, _u32, _u64, ctypes.c_double, _dp, _i32, _dp,
                                     _i32, _i32, _vp, _vp, ctypes.POINTER(DymuCostState), _vp,
                                     _vp]),
    "dymu_pack_speed": (_i32, [_vp, _u32, _u32, _u64, ctypes.c_double,
                               ctypes.POINTER(DymuCostState), _vp, _vp]),
    "dymu_resolve_window_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _u32, _u32, _u32,
                                          _u32, _u32, _u32, _vp, ctypes.POINTER(DymuStats)]),
    "dymu_update_window_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _u32, _u32, _u32,
                                         _u32, _u32, _u32, _i32, _vp,
                                         ctypes.POINTER(DymuStats)]),
    "dymu_resolve_window": (_i32, [_vp, _dp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _u32,
                                   _dp, ctypes.POINTER(DymuStats)]),
    "dymu_solve_until_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _u32, _u32, _u32, _u32,
                                       _vp, ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(DymuStats)]),
    "dymu_early_exit_mask": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, ctypes.c_double, _vp, _u64,
                                    ctypes.POINTER(_u64), _vp]),
    "dymu_scatter": (_i32, [_vp, _vp, _u32, _u64, _vp, _vp, _u64, _vp]),
    "dymu_region_stats": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _u32, _u32, ctypes.c_double,
                                 ctypes.c_double, ctypes.c_double, ctypes.POINTER(DymuRegion),
                                 _vp]),
    "dymu_extract_paths_device": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double, _u32, _u32,
                                         ctypes.c_double, _vp, _u32, _u32, _u32, _vp, _vp, _vp,
                                         _vp]),
    "dymu_last_paths_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_solve_seeds_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _vp, _u32, _vp,
                                       ctypes.POINTER(DymuStats)]),
    "dymu_goal_labels_device": (_i32, [_vp, _vp, _u32, _u32, _u64, _vp, _u32, _vp, _vp,
                                       ctypes.POINTER(_u32)]),
    "dymu_extract_paths_goals_device": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double, _vp,
                                               _vp, _u32, ctypes.c_double, _vp, _u32, _u32, _u32,
                                               _vp, _vp, _vp, _vp, _vp]),
    "dymu_last_labels_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_path_stats_device": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double, _u32, _u32,
                                      _vp, _vp, _u32, ctypes.c_double, _vp, _u32, _u32, _vp, _vp,
                                      _u32, _u32, _vp, _vp]),
    "dymu_last_path_stats_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_arrive_paths_device": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double, _u32, _u32,
                                        _vp, _vp, _u32, ctypes.c_double, _vp, _u32, _u32, _u32,
                                        _vp, _vp, _vp, _vp]),
    "dymu_last_arrive_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_arrive_simplified_device": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double, _u32,
                                             _u32, _vp, _vp, _u32, ctypes.c_double, _vp, _u32,
                                             ctypes.c_double, _u32, _u32, _vp, _vp, _vp, _vp,
                                             _vp]),
    "dymu_last_arrive_simplified_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_route_fields_workspace": (ctypes.c_size_t, [_u32, _u32, _u32,
                                                      ctypes.POINTER(DymuRouteOut)]),
    "dymu_route_fields_device": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double, _vp, _u32,
                                        _vp, _vp, _u32, ctypes.POINTER(DymuRouteOut), _vp,
                                        ctypes.c_size_t, _vp, ctypes.POINTER(_u32)]),
    "dymu_last_route_fields_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_last_route_fields_stages": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_route_usage_workspace": (ctypes.c_size_t, [_u32, _u32, ctypes.POINTER(DymuUsageOut)]),
    "dymu_route_usage_device": (_i32, [_vp, _vp, _u32, _u32, _u64, _vp, _u32, _vp, _u64,
                                       ctypes.POINTER(DymuUsageOut), _vp, _vp, ctypes.c_size_t,
                                       _vp, ctypes.POINTER(_u32)]),
    "dymu_last_route_usage_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_last_route_usage_stages": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_last_route_usage_round_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(_u32)]),
    "dymu_batch_plane_rows": (_u32, [_u32]),
    "dymu_stack_speed_device": (_i32, [_vp, _vp, _u64, _u64, _u32, _u32, _u32, _vp, _u64, _vp]),
    "dymu_solve_batch_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _u64, _vp, _u32, _vp,
                                       ctypes.POINTER(DymuStats)]),
    "dymu_gather_costs_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _u64, ctypes.c_double, _vp,
                                        _u32, _vp, _vp]),
    "dymu_update_seeds_window_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _vp, _u32, _u32,
                                               _u32, _u32, _u32, _i32, _vp,
                                               ctypes.POINTER(DymuStats)]),
    "dymu_update_batch_window_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _u64, _vp, _u32,
                                               _vp, _u32, _i32, _vp, ctypes.POINTER(DymuStats)]),
    "dymu_solve_seeds_until_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _vp, _u32, _vp, _u32,
                                             _vp, ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(DymuStats)]),
    "dymu_solve_batch_until_device": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _u64, _vp, _u32,
                                             _vp, _u32, _vp, ctypes.POINTER(ctypes.c_double),
                                             _vp, ctypes.POINTER(DymuStats)]),
    "dymu_clearance_device": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, ctypes.c_double, _vp,
                                     ctypes.POINTER(DymuStats)]),
    "dymu_clearance_update_device": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, ctypes.c_double,
                                            _u32, _u32, _u32, _u32, _vp, ctypes.POINTER(_u32),
                                            ctypes.POINTER(DymuStats)]),
    "dymu_clearance_edit_device": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, ctypes.c_double,
                                          _u32, _u32, _u32, _u32, _vp, ctypes.POINTER(_u32),
                                          ctypes.POINTER(DymuStats)]),
    "dymu_inflate_speed_device": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u64, ctypes.c_double,
                                         _vp]),
    "dymu_batch_reduce_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _u64, _i32, _vp, _u32, _vp, _vp,
                                        _vp, _u64, _vp, _u64, ctypes.POINTER(DymuReduceSummary),
                                        _vp]),
    "dymu_last_reduce_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_level_mask_device": (_i32, [_vp, _vp, _u32, _u32, _u64, ctypes.c_double, _vp, _u64,
                                      ctypes.POINTER(DymuRegion), _vp]),
    "dymu_device_alloc_cached": (_i32, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "dymu_memcpy2d_d2h": (_i32, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                 ctypes.c_size_t, ctypes.c_size_t]),
    "dymu_memcpy2d_h2d": (_i32, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                 ctypes.c_size_t, ctypes.c_size_t]),
    "dymu_host_register": (_i32, [_vp, _vp, ctypes.c_size_t]),
    "dymu_host_unregister": (_i32, [_vp, _vp]),
    "dymu_get_stream": (_vp, [_vp]),
    "dymu_strerror": (ctypes.c_char_p, [_i32]),
    "dymu_last_error": (ctypes.c_char_p, [_vp]),
    "dymu_abi_version": (_i32, []),
    "dymu_device_count": (_i32, []),
}

_fim = None


def lib_path(name: str) -> str:
    return os.path.join(_LIBDIR, name)


def load_fim() -> ctypes.CDLL:
    """Load libdymu_fim.so (RTLD_GLOBAL so the planner library resolves it)."""
    global _fim
    if _fim is None:
        path = lib_path("libdymu_fim.so")
        if not os.path.exists(path):
            raise DymuError(-5, f"HIP extension missing: {path} (run __graft_entry__.build())")
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        ab_build = "DYMU_LIBDIR" in os.environ  # an older A/B build may lack newer symbols
        for name, (res, args) in FIM_SYMBOLS.items():
            if ab_build and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _fim = lib
    return _fim


def _check(rc: int, ctx=None):
    if rc != DYMU_OK:
        what = ""
        if ctx is not None:
            msg = load_fim().dymu_last_error(ctx)
            what = msg.decode() if msg else ""
        raise DymuError(rc, what)


@dataclass
class SolveResult:
    T: np.ndarray
    stats: dict


class Engine:
    """One HIP context (stream + workspace) on one device."""

    def __init__(self, device: int = -1, passes_per_check: int = 0, max_passes: int = 0,
                 max_inner: int = 0, grid_blocks: int = 0, kernel: int = 0,
                 prio_target: int = 0, exact_sqrt: int = 0, deterministic: int = 0):
        lib = load_fim()
        self._lib = lib
        opts = DymuOpts(device, passes_per_check, max_passes, max_inner, grid_blocks, kernel,
                        prio_target, exact_sqrt, deterministic)
        ctx = _vp()
        rc = lib.dymu_create(ctypes.byref(ctx), ctypes.byref(opts))
        if rc != DYMU_OK:
            raise DymuError(rc, "dymu_create")
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            self._lib.dymu_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- host-buffer solve (planner path) --
    def solve(self, F: np.ndarray, goal_i: int, goal_j: int) -> SolveResult:
        F = np.ascontiguousarray(F, dtype=np.float64)
        if F.ndim != 2:
            raise ValueError("F must be 2-D [ny, nx]")
        ny, nx = F.shape
        T = np.empty_like(F)
        st = DymuStats()
        _check(self._lib.dymu_solve(self.ctx, F, nx, ny, goal_i, goal_j, T, ctypes.byref(st)),
               self.ctx)
        return SolveResult(T, st.as_dict())

    def resolve_window(self, F: np.ndarray, goal_i: int, goal_j: int, i0: int, j0: int, w: int,
                       h: int) -> SolveResult:
        """Windowed re-propagation after F changed inside [i0,i0+w) x [j0,j0+h);
        the previous solve on this engine must be of the same grid and goal."""
        F = np.ascontiguousarray(F, dtype=np.float64)
        ny, nx = F.shape
        T = np.empty_like(F)
        st = DymuStats()
        _check(self._lib.dymu_resolve_window(self.ctx, F, nx, ny, goal_i, goal_j, i0, j0, w, h, T,
                                             ctypes.byref(st)), self.ctx)
        return SolveResult(T, st.as_dict())

    def resolve_window_device(self, dF: int, dT: int, nx: int, ny: int, ld: int, goal_i: int,
                              goal_j: int, i0: int, j0: int, w: int, h: int,
                              stream: int = 0) -> dict:
        st = DymuStats()
        _check(self._lib.dymu_resolve_window_device(self.ctx, dF, dT, nx, ny, ld, goal_i, goal_j,
                                                    i0, j0, w, h, stream or None,
                                                    ctypes.byref(st)), self.ctx)
        return st.as_dict()

    def update_window_device(self, dF: int, dT: int, nx: int, ny: int, ld: int, goal_i: int,
                             goal_j: int, i0: int, j0: int, w: int, h: int,
                             decrease_only: bool, stream: int = 0) -> dict:
        st = DymuStats()
        _check(self._lib.dymu_update_window_device(self.ctx, dF, dT, nx, ny, ld, goal_i, goal_j,
                                                   i0, j0, w, h, int(bool(decrease_only)),
                                                   stream or None, ctypes.byref(st)), self.ctx)
        return st.as_dict()

    # -- device-resident solve --
    def solve_device(self, dF: int, dT: int, nx: int, ny: int, ld: int, goal_i: int,
                     goal_j: int, stream: int = 0) -> dict:
        st = DymuStats()
        _check(self._lib.dymu_solve_device(self.ctx, dF, dT, nx, ny, ld, goal_i, goal_j,
                                           stream or None, ctypes.byref(st)), self.ctx)
        return st.as_dict()

    def solve_until_device(self, dF: int, dT: int, nx: int, ny: int, ld: int, goal_i: int,
                           goal_j: int, start_i: int, start_j: int, stream: int = 0):
        """computeTotalCostMap's propagation: stops once the start and its nb4 are final.
        Returns (t_closed, stats)."""
        st = DymuStats()
        tc = ctypes.c_double()
        _check(self._lib.dymu_solve_until_device(self.ctx, dF, dT, nx, ny, ld, goal_i, goal_j,
                                                 start_i, start_j, stream or None,
                                                 ctypes.byref(tc), ctypes.byref(st)), self.ctx)
        return tc.value, st.as_dict()

    def synth_speed(self, dF: int, nx: int, ny: int, ld: int, row0: int = 0, seed: int = 1,
                    obst_frac: float = 0.0, obst_seed: int = 3, goal_i: int = 0,
                    goal_j: int = 0, stream: int = 0):
        _check(self._lib.dymu_synth_speed(self.ctx, dF, nx, ny, ld, row0, seed, obst_frac,
                                          obst_seed, goal_i, goal_j, stream or None), self.ctx)

    def find_equal(self, dT: int, nx: int, ny: int, ld: int, value: float, cap: int):
        """Cells whose value is bitwise `value` (dymu_find_equal): (count, indices of the
        first min(count, cap) of them, j * nx + i, in no particular order)."""
        idx = np.zeros(max(1, cap), dtype=np.uint64)
        n = _u64()
        _check(self._lib.dymu_find_equal(self.ctx, dT, nx, ny, ld, float(value), idx.ctypes.data,
                                         cap, ctypes.byref(n), None), self.ctx)
        return n.value, idx[:min(n.value, cap)]

    def count_equal(self, dT: int, nx: int, ny: int, ld: int, value: float) -> int:
        """The number of cells whose value is bitwise `value` (dymu_count_equal)."""
        n = _u64()
        _check(self._lib.dymu_count_equal(self.ctx, dT, nx, ny, ld, float(value),
                                          ctypes.byref(n), None), self.ctx)
        return n.value

    def early_exit_mask(self, dF: int, dT: int, nx: int, ny: int, ld: int, tc: float, cap: int):
        """dymu_early_exit_mask on the device map dT: (n_band, indices j * nx + i of the
        first min(n_band, cap) band cells, in no particular order).  cap = 0 passes no
        buffer: the map is masked and only the count comes back."""
        idx = np.zeros(cap, dtype=np.uint64)
        n = _u64()
        _check(self._lib.dymu_early_exit_mask(self.ctx, dF, dT, nx, ny, ld, float(tc),
                                              idx.ctypes.data if cap else None, cap,
                                              ctypes.byref(n), None), self.ctx)
        return n.value, idx[:min(n.value, cap)]

    def scatter(self, dT: int, nx: int, ld: int, idx: np.ndarray, vals: np.ndarray):
        """T[idx // nx, idx % nx] = vals on the device (dymu_scatter)."""
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if idx.shape != vals.shape:
            raise ValueError("idx and vals differ in shape")
        _check(self._lib.dymu_scatter(self.ctx, dT, nx, ld, idx.ctypes.data, vals.ctypes.data,
                                      idx.size, None), self.ctx)

    def region_stats(self, dF: int, dT: int, nx: int, ny: int, ld: int, goal_i: int,
                     goal_j: int, thr: float, lo: float, hi: float) -> dict:
        """dymu_region_stats: bounding box (inclusive) of the cells with T <= thr, the
        number with lo <= T <= hi, the distance from the goal to the nearest cell of
        another speed."""
        r = DymuRegion()
        _check(self._lib.dymu_region_stats(self.ctx, dF, dT, nx, ny, ld, goal_i, goal_j, thr, lo,
                                           hi, ctypes.byref(r), None), self.ctx)
        return {"box": (r.i0, r.j0, r.i1, r.j1), "n_range": r.n_range, "r_const": r.r_const}

    def extract_paths(self, dT: int, nx: int, ny: int, ld: int, res: float, goal_i: int,
                      goal_j: int, tau: float, starts_xy, max_wp: int, stride: int = 1,
                      stream: int = 0):
        """dymu_extract_paths_device on the device map dT for host starts (n, 2) in
        grid-local metres: (out [n, max_wp, 4] of x, y, dcx, dcy; counts [n]; status [n])."""
        xy = np.ascontiguousarray(starts_xy, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        out = np.zeros((n, max_wp, 4))
        cnt = np.zeros(n, dtype=np.int32)
        st = np.zeros(n, dtype=np.int32)
        if n == 0:
            return out, cnt, st
        ptrs = [self.alloc(xy.nbytes), self.alloc(out.nbytes), self.alloc(4 * n),
                self.alloc(4 * n)]
        try:
            self.h2d(ptrs[0], xy)
            _check(self._lib.dymu_extract_paths_device(
                self.ctx, dT, nx, ny, ld, res, goal_i, goal_j, tau, ptrs[0], n, max_wp, stride,
                ptrs[1], ptrs[2], ptrs[3], stream or None), self.ctx)
            if stream:  # d2h is ordered on the context stream only
                self.last_paths_ms()
            self.d2h(cnt, ptrs[2])
            self.d2h(st, ptrs[3])
            self.d2h(out, ptrs[1])
        finally:
            for p in ptrs:
                self.free(p)
        for q in range(n):  # slots past the count were never written
            out[q, max(cnt[q], 0):] = 0.0
        return out, cnt, st

    def last_paths_ms(self) -> float:
        """Device time of the last extract_paths kernel (waits for it)."""
        ms = ctypes.c_double()
        _check(self._lib.dymu_last_paths_ms(self.ctx, ctypes.byref(ms)), self.ctx)
        return ms.value

    # -- goal sets --
    @staticmethod
    def _seeds(seeds) -> np.ndarray:
        """(i, j[, t0]) rows as an array of dymu_seed."""
        a = np.zeros(len(seeds), dtype=SEED_DTYPE)
        for k, s in enumerate(seeds):
            a[k] = (int(s[0]), int(s[1]), float(s[2]) if len(s) > 2 else 0.0)
        return a

    def solve_seeds_device(self, dF: int, dT: int, nx: int, ny: int, ld: int, seeds,
                           stream: int = 0) -> dict:
        """dymu_solve_seeds_device: the converged multi-source solve of the seeds
        (i, j[, t0]) into dT."""
        a = self._seeds(seeds)
        st = DymuStats()
        _check(self._lib.dymu_solve_seeds_device(self.ctx, dF, dT, nx, ny, ld, a.ctypes.data,
                                                 len(a), stream or None, ctypes.byref(st)),
               self.ctx)
        return st.as_dict()

    def goal_labels_device(self, dT: int, nx: int, ny: int, ld: int, seeds, d_label: int = 0,
                           stream: int = 0, download: bool = True):
        """dymu_goal_labels_device on the device map dT: (labels [ny, nx] uint32, rounds).
        With d_label (nx * ny words of device memory) the labels stay there as well, and
        download=False then returns (None, rounds) without the copy to the host."""
        a = self._seeds(seeds)
        rounds = _u32()
        own = 0 if d_label else self.alloc_cached(4 * nx * ny)
        try:
            _check(self._lib.dymu_goal_labels_device(self.ctx, dT, nx, ny, ld, a.ctypes.data,
                                                     len(a), d_label or own, stream or None,
                                                     ctypes.byref(rounds)), self.ctx)
            lab = None
            if download or own:
                lab = np.empty((ny, nx), dtype=np.uint32)
                self.d2h(lab, d_label or own)
        finally:
            if own:
                self.free(own)
        return lab, rounds.value

    def last_labels_ms(self) -> float:
        """Device time of the last goal_labels_device (first kernel to last)."""
        ms = ctypes.c_double()
        _check(self._lib.dymu_last_labels_ms(self.ctx, ctypes.byref(ms)), self.ctx)
        return ms.value

    def extract_paths_goals(self, dT: int, nx: int, ny: int, ld: int, res: float, d_label: int,
                            goals_ij, tau: float, starts_xy, max_wp: int, stride: int = 1,
                            stream: int = 0):
        """dymu_extract_paths_goals_device: extract_paths with the sink taken from the label
        map d_label (device) and the goals' cells goals_ij (n_goals, 2): (out, counts,
        status, sinks [n] int32)."""
        xy = np.ascontiguousarray(starts_xy, dtype=np.float64).reshape(-1, 2)
        gxy = res * np.ascontiguousarray(goals_ij, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        out = np.zeros((n, max_wp, 4))
        cnt = np.zeros(n, dtype=np.int32)
        st = np.zeros(n, dtype=np.int32)
        sink = np.full(n, -1, dtype=np.int32)
        if n == 0:
            return out, cnt, st, sink
        ptrs = [self.alloc(xy.nbytes), self.alloc(out.nbytes), self.alloc(4 * n),
                self.alloc(4 * n), self.alloc(4 * n), self.alloc(gxy.nbytes)]
        try:
            self.h2d(ptrs[0], xy)
            self.h2d(ptrs[5], gxy)
            _check(self._lib.dymu_extract_paths_goals_device(
                self.ctx, dT, nx, ny, ld, res, d_label, ptrs[5], len(gxy), tau, ptrs[0], n,
                max_wp, stride, ptrs[1], ptrs[2], ptrs[3], stream or None, ptrs[4]), self.ctx)
            if stream:  # d2h is ordered on the context stream only
                self.last_paths_ms()
            self.d2h(cnt, ptrs[2])
            self.d2h(st, ptrs[3])
            self.d2h(sink, ptrs[4])
            self.d2h(out, ptrs[1])
        finally:
            for p in ptrs:
                self.free(p)
        for q in range(n):  # slots past the count were never written
            out[q, max(cnt[q], 0):] = 0.0
        return out, cnt, st, sink

    # -- per-path summaries --
    def path_stats(self, dT: int, nx: int, ny: int, ld: int, res: float, goal_i: int,
                   goal_j: int, tau: float, starts_xy, max_wp: int, fields=(), n_lanes: int = 0,
                   d_label: int = 0, goals_ij=None, stream: int = 0) -> np.ndarray:
        """dymu_path_stats_device on the device map dT for host starts (n, 2) in grid-local
        metres: a PATH_STAT_DTYPE array of n records.  fields: up to PATH_FIELDS pairs
        (device pointer, pitch) of sampled maps; n_lanes: the lanes of the kernel's grid (0:
        the default); d_label with goals_ij (n_goals, 2): the sink follows the label map."""
        xy = np.ascontiguousarray(starts_xy, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        out = np.zeros(n, dtype=PATH_STAT_DTYPE)
        fp = (_vp * max(len(fields), 1))(*[int(f[0]) for f in fields])
        fl = (_u64 * max(len(fields), 1))(*[int(f[1]) for f in fields])
        gxy = None
        if d_label:
            gxy = res * np.ascontiguousarray(goals_ij, dtype=np.float64).reshape(-1, 2)
        ptrs = [self.alloc(max(xy.nbytes, 8)), self.alloc(max(out.nbytes, 8))]
        if gxy is not None:
            ptrs.append(self.alloc(max(gxy.nbytes, 8)))
        try:
            if n:
                self.h2d(ptrs[0], xy)
            if gxy is not None and len(gxy):
                self.h2d(ptrs[2], gxy)
            _check(self._lib.dymu_path_stats_device(
                self.ctx, dT, nx, ny, ld, res, goal_i, goal_j, d_label or None,
                ptrs[2] if gxy is not None else None, len(gxy) if gxy is not None else 0, tau,
                ptrs[0], n, max_wp, ctypes.cast(fp, _vp), ctypes.cast(fl, _vp), len(fields),
                n_lanes, ptrs[1], stream or None), self.ctx)
            if n:
                if stream:  # d2h is ordered on the context stream only
                    self.last_path_stats_ms()
                self.d2h(out, ptrs[1])
        finally:
            for p in ptrs:
                self.free(p)
        return out

    def last_path_stats_ms(self) -> float:
        """Device time of the last path_stats kernel (waits for it)."""
        ms = ctypes.c_double()
        _check(self._lib.dymu_last_path_stats_ms(self.ctx, ctypes.byref(ms)), self.ctx)
        return ms.value

    # -- the arriving descent --
    def arrive_paths(self, dT: int, nx: int, ny: int, ld: int, res: float, goal_i: int,
                     goal_j: int, tau: float, starts_xy, max_wp: int, stride: int = 1,
                     store: bool = True, d_label: int = 0, goals_ij=None, stream: int = 0):
        """dymu_arrive_paths_device on the device map dT for host starts (n, 2) in grid-local
        metres: (out [n, max_wp, 4] of x, y, dcx, dcy; counts [n]; records, an
        ARRIVE_STAT_DTYPE array).  store=False passes d_out = NULL: (None, None, records).
        d_label with goals_ij (n_goals, 2): the sink follows the label map."""
        xy = np.ascontiguousarray(starts_xy, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        rec = np.zeros(n, dtype=ARRIVE_STAT_DTYPE)
        out = np.zeros((n, max_wp, 4)) if store else None
        cnt = np.zeros(n, dtype=np.int32) if store else None
        gxy = None
        if d_label:
            gxy = res * np.ascontiguousarray(goals_ij, dtype=np.float64).reshape(-1, 2)
        ptrs = [self.alloc(max(xy.nbytes, 8)), self.alloc(max(rec.nbytes, 8)),
                self.alloc(max(out.nbytes, 8)) if store else 0,
                self.alloc(4 * max(n, 1)) if store else 0,
                self.alloc(max(gxy.nbytes, 8)) if gxy is not None else 0]
        try:
            if n:
                self.h2d(ptrs[0], xy)
            if gxy is not None and len(gxy):
                self.h2d(ptrs[4], gxy)
            _check(self._lib.dymu_arrive_paths_device(
                self.ctx, dT, nx, ny, ld, res, goal_i, goal_j, d_label or None, ptrs[4] or None,
                len(gxy) if gxy is not None else 0, tau, ptrs[0], n, max_wp, stride,
                ptrs[2] or None, ptrs[3] if store else None, ptrs[1], stream or None), self.ctx)
            if n:
                if stream:  # d2h is ordered on the context stream only
                    self.last_arrive_ms()
                self.d2h(rec, ptrs[1])
                if store:
                    self.d2h(cnt, ptrs[3])
                    self.d2h(out, ptrs[2])
        finally:
            for p in ptrs:
                if p:
                    self.free(p)
        if store:
            for q in range(n):  # slots past the count were never written
                out[q, max(cnt[q], 0):] = 0.0
        return out, cnt, rec

    def last_arrive_ms(self) -> float:
        """Device time of the last arrive_paths kernel (waits for it)."""
        ms = ctypes.c_double()
        _check(self._lib.dymu_last_arrive_ms(self.ctx, ctypes.byref(ms)), self.ctx)
        return ms.value

    # -- the simplified arriving descent --
    def arrive_simplified(self, dT: int, nx: int, ny: int, ld: int, res: float, goal_i: int,
                          goal_j: int, tau: float, starts_xy, eps: float, max_steps: int,
                          max_kept: int, store: bool = True, with_index: bool = True,
                          d_label: int = 0, goals_ij=None, stream: int = 0):
        """dymu_arrive_simplified_device on the device map dT for host starts (n, 2) in
        grid-local metres: (out [n, max_kept, 4] of x, y, dcx, dcy; index [n, max_kept]
        uint32; counts [n]; records).  counts[q] is what the rule keeps, stored or not:
        only the first max_kept have a slot, the rest of out and index is zero.
        store=False passes d_out = NULL, with_index=False d_index = NULL (None returned)."""
        xy = np.ascontiguousarray(starts_xy, dtype=np.float64).reshape(-1, 2)
        n = len(xy)
        rec = np.zeros(n, dtype=ARRIVE_STAT_DTYPE)
        out = np.zeros((n, max_kept, 4)) if store else None
        idx = np.zeros((n, max_kept), dtype=np.uint32) if with_index else None
        cnt = np.zeros(n, dtype=np.int32)
        gxy = None
        if d_label:
            gxy = res * np.ascontiguousarray(goals_ij, dtype=np.float64).reshape(-1, 2)
        ptrs = [self.alloc(max(xy.nbytes, 8)), self.alloc(max(rec.nbytes, 8)),
                self.alloc(max(out.nbytes, 8)) if store else 0,
                self.alloc(max(idx.nbytes, 8)) if with_index else 0,
                self.alloc(4 * max(n, 1)),
                self.alloc(max(gxy.nbytes, 8)) if gxy is not None else 0]
        try:
            if n:
                self.h2d(ptrs[0], xy)
            if gxy is not None and len(gxy):
                self.h2d(ptrs[5], gxy)
            _check(self._lib.dymu_arrive_simplified_device(
                self.ctx, dT, nx, ny, ld, res, goal_i, goal_j, d_label or None, ptrs[5] or None,
                len(gxy) if gxy is not None else 0, tau, ptrs[0], n, eps, max_steps, max_kept,
                ptrs[2] or None, ptrs[3] or None, ptrs[4], ptrs[1], stream or None), self.ctx)
            if n:
                if stream:  # d2h is ordered on the context stream only
                    self.last_arrive_simplified_ms()
                self.d2h(rec, ptrs[1])
                self.d2h(cnt, ptrs[4])
                if store and out.size:
                    self.d2h(out, ptrs[2])
                if with_index and idx.size:
                    self.d2h(idx, ptrs[3])
        finally:
            for p in ptrs:
                if p:
                    self.free(p)
        for q in range(n):  # slots past the count were never written
            if store:
                out[q, max(cnt[q], 0):] = 0.0
            if with_index:
                idx[q, max(cnt[q], 0):] = 0
        return out, idx, cnt, rec

    def last_arrive_simplified_ms(self) -> float:
        """Device time of the last arrive_simplified kernel (waits for it)."""
        ms = ctypes.c_double()
        _check(self._lib.dymu_last_arrive_simplified_ms(self.ctx, ctypes.byref(ms)), self.ctx)
        return ms.value

    # -- batched solves --
    def stack_speed(self, src: int, src_ld: int, src_plane_stride: int, nx: int, ny: int,
                    B: int, dF_stack: int, ld: int, stream: int = 0):
        """dymu_stack_speed_device: the stacked speed of B planes (B * batch_plane_rows(ny)
        rows of pitch ld) from the maps at src + b * src_plane_stride (0: one shared map),
        wall rows +inf."""
        _check(self._lib.dymu_stack_speed_device(self.ctx, src, src_ld, src_plane_stride, nx,
                                                 ny, B, dF_stack, ld, stream or None), self.ctx)

    def solve_batch_device(self, dF_stack: int, dT_stack: int, nx: int, ny: int, B: int,
                           ld: int, seeds, stream: int = 0) -> dict:
        """dymu_solve_batch_device: every plane of the stack converged from its own seeds
        (plane, i, j[, t0]) in one pass sequence."""
        a = np.zeros(len(seeds), dtype=BATCH_SEED_DTYPE)
        for k, s in enumerate(seeds):
            a[k] = (int(s[0]), int(s[1]), int(s[2]), 0, float(s[3]) if len(s) > 3 else 0.0)
        st = DymuStats()
        _check(self._lib.dymu_solve_batch_device(self.ctx, dF_stack, dT_stack, nx, ny, B, ld,
                                                 a.ctypes.data, len(a), stream or None,
                                                 ctypes.byref(st)), self.ctx)
        return st.as_dict()

    # -- early exit on target cells --
    def solve_seeds_until_device(self, dF: int, dT: int, nx: int, ny: int, ld: int, seeds,
                                 targets, stream: int = 0):
        """dymu_solve_seeds_until_device: solve_seeds_device that stops once the target
        cells (i, j) of finite speed are final.  Returns (t_closed, stats)."""
        a = self._seeds(seeds)
        tg = np.zeros(len(targets), dtype=CELL_DTYPE)
        for k, q in enumerate(targets):
            tg[k] = (int(q[0]), int(q[1]))
        st = DymuStats()
        tc = ctypes.c_double()
        _check(self._lib.dymu_solve_seeds_until_device(
            self.ctx, dF, dT, nx, ny, ld, a.ctypes.data if len(a) else None, len(a),
            tg.ctypes.data if len(tg) else None, len(tg), stream or None, ctypes.byref(tc),
            ctypes.byref(st)), self.ctx)
        return tc.value, st.as_dict()

    def solve_batch_until_device(self, dF_stack: int, dT_stack: int, nx: int, ny: int, B: int,
                                 ld: int, seeds, targets, stream: int = 0):
        """dymu_solve_batch_until_device: solve_batch_device that stops once the target
        cells (plane, i, j) of finite speed are final in every plane.  Returns (t_closed,
        t_plane [B], stats)."""
        a = np.zeros(len(seeds), dtype=BATCH_SEED_DTYPE)
        for k, s in enumerate(seeds):
            a[k] = (int(s[0]), int(s[1]), int(s[2]), 0, float(s[3]) if len(s) > 3 else 0.0)
        tg = np.zeros(len(targets), dtype=BATCH_CELL_DTYPE)
        for k, q in enumerate(targets):
            tg[k] = (int(q[0]), int(q[1]), int(q[2]), 0)
        st = DymuStats()
        tc = ctypes.c_double()
        tp = np.zeros(max(int(B), 1))
        _check(self._lib.dymu_solve_batch_until_device(
            self.ctx, dF_stack, dT_stack, nx, ny, B, ld, a.ctypes.data if len(a) else None,
            len(a), tg.ctypes.data if len(tg) else None, len(tg), stream or None,
            ctypes.byref(tc), tp.ctypes.data, ctypes.byref(st)), self.ctx)
        return tc.value, tp[:B].copy(), st.as_dict()

    # -- obstacle clearance field and risk-inflated speed --
    def clearance_device(self, dF: int, dW: int, dS: int, nx: int, ny: int, ld: int, c: float,
                         stream: int = 0) -> dict:
        """dymu_clearance_device: dS = the multi-source solution on the constant speed c with
        every obstacle cell of dF (+inf or NaN) seeded at 0, exact up to the level 1; dW is
        a work map of the same shape."""
        st = DymuStats()
        _check(self._lib.dymu_clearance_device(self.ctx, dF, dW, dS, nx, ny, ld, c,
                                               stream or None, ctypes.byref(st)), self.ctx)
        return st.as_dict()

    def clearance_update_device(self, dF: int, dW: int, dS: int, nx: int, ny: int, ld: int,
                                c: float, i0: int, j0: int, w: int, h: int,
                                stream: int = 0) -> dict:
        """dymu_clearance_update_device: dS, the field clearance_device left for an old mask
        (dW still holding c), brought to the mask of dF, which adds obstacle cells inside
        the window only.  Returns the stats with "box": (i0, j0, w, h) of the cells the call
        may have written."""
        st = DymuStats()
        box = (_u32 * 4)()
        _check(self._lib.dymu_clearance_update_device(self.ctx, dF, dW, dS, nx, ny, ld, c, i0, j0,
                                                      w, h, stream or None, box,
                                                      ctypes.byref(st)), self.ctx)
        d = st.as_dict()
        d["box"] = tuple(int(v) for v in box)
        return d

    def clearance_edit_device(self, dF: int, dW: int, dS: int, nx: int, ny: int, ld: int,
                              c: float, i0: int, j0: int, w: int, h: int,
                              stream: int = 0) -> dict:
        """dymu_clearance_edit_device: clearance_update_device for a window that may free
        obstacle cells as well as add them: the field is raised where the freed cells
        supported it, then re-propagated.  Returns the stats with "box": (i0, j0, w, h) of the
        cells the call may have written; last_update_stats() holds the raise's figures."""
        st = DymuStats()
        box = (_u32 * 4)()
        _check(self._lib.dymu_clearance_edit_device(self.ctx, dF, dW, dS, nx, ny, ld, c, i0, j0,
                                                    w, h, stream or None, box,
                                                    ctypes.byref(st)), self.ctx)
        d = st.as_dict()
        d["box"] = tuple(int(v) for v in box)
        return d

    def inflate_speed(self, dF: int, dS: int, dOut: int, nx: int, ny: int, ld: int,
                      risk_ratio: float, stream: int = 0):
        """dymu_inflate_speed_device: dOut = dF * (risk_ratio * max(1 - dS, 0) + 1); dOut may
        be dF."""
        _check(self._lib.dymu_inflate_speed_device(self.ctx, dF, dS, dOut, nx, ny, ld,
                                                   risk_ratio, stream or None), self.ctx)

    # -- windowed updates of seeded maps and stacks --
    def update_seeds_window_device(self, dF: int, dT: int, nx: int, ny: int, ld: int, seeds,
                                   i0: int, j0: int, w: int, h: int,
                                   decrease_only: bool = False, stream: int = 0) -> dict:
        """dymu_update_seeds_window_device: dT, the converged map of the seeds (i, j[, t0])
        under the old speed, brought to the new speed dF, changed only inside the window."""
        a = self._seeds(seeds)
        st = DymuStats()
        _check(self._lib.dymu_update_seeds_window_device(
            self.ctx, dF, dT, nx, ny, ld, a.ctypes.data if len(a) else None, len(a), i0, j0, w,
            h, int(bool(decrease_only)), stream or None, ctypes.byref(st)), self.ctx)
        return st.as_dict()

    def update_batch_window_device(self, dF_stack: int, dT_stack: int, nx: int, ny: int, B: int,
                                   ld: int, seeds, windows, decrease_only: bool = False,
                                   stream: int = 0) -> dict:
        """dymu_update_batch_window_device: the solved stack of solve_batch_device (same
        seeds (plane, i, j[, t0])) brought to the new stacked speed, changed only inside
        the windows (plane, i0, j0, w, h) -- any number per plane, none included."""
        a = np.zeros(len(seeds), dtype=BATCH_SEED_DTYPE)
        for k, s in enumerate(seeds):
            a[k] = (int(s[0]), int(s[1]), int(s[2]), 0, float(s[3]) if len(s) > 3 else 0.0)
        wn = np.zeros(len(windows), dtype=BATCH_WINDOW_DTYPE)
        for k, q in enumerate(windows):
            wn[k] = (int(q[0]), int(q[1]), int(q[2]), int(q[3]), int(q[4]), 0)
        st = DymuStats()
        _check(self._lib.dymu_update_batch_window_device(
            self.ctx, dF_stack, dT_stack, nx, ny, B, ld, a.ctypes.data if len(a) else None,
            len(a), wn.ctypes.data if len(wn) else None, len(wn), int(bool(decrease_only)),
            stream or None, ctypes.byref(st)), self.ctx)
        return st.as_dict()

    def gather_costs(self, dT_stack: int, nx: int, ny: int, B: int, ld: int, res: float,
                     points_xy, stream: int = 0) -> np.ndarray:
        """dymu_gather_costs_device for host points (M, 2) in grid-local metres: [B, M], the
        planner's getTotalCost of every point on every plane of the solved stack."""
        xy = np.ascontiguousarray(points_xy, dtype=np.float64).reshape(-1, 2)
        M = len(xy)
        out = np.zeros((B, M))
        if M == 0:
            return out
        ptrs = [self.alloc(xy.nbytes), self.alloc(out.nbytes)]
        try:
            self.h2d(ptrs[0], xy)
            _check(self._lib.dymu_gather_costs_device(self.ctx, dT_stack, nx, ny, B, ld, res,
                                                      ptrs[0], M, ptrs[1], None), self.ctx)
            self.d2h(out, ptrs[1])
        finally:
            for p in ptrs:
                self.free(p)
        return out

    # -- plane reduction and level mask --
    def batch_reduce(self, dT_stack: int, nx: int, ny: int, B: int, ld: int, op, planes=None,
                     weights=None, offsets=None, d_out: int = 0, out_ld: int = 0, d_arg: int = 0,
                     arg_ld: int = 0, summary: bool = True, stream: int = 0):
        """dymu_batch_reduce_device: d_out = the fold `op` ("sum" / "max" / "min" or 0 / 1 / 2)
        of every cell over the listed planes of the stack (None: all), each optionally
        weighted and offset; d_arg (MAX / MIN, optional) the plane that gave the cell.
        Returns the summary of d_out as a dict (the call then synchronises), or None with
        summary=False (asynchronous)."""
        pl = None if planes is None else np.ascontiguousarray(planes, dtype=np.uint32).ravel()
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).ravel()
        o = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64).ravel()
        n = B if pl is None else len(pl)
        for a in (w, o):
            if a is not None and len(a) != n:
                raise DymuError(-1, "one weight / offset per listed plane")
        # an empty list stays a list (n_planes = 0 with a list is an argument error)
        keep = np.zeros(1, dtype=np.uint32) if pl is not None and len(pl) == 0 else pl
        s = DymuReduceSummary()
        _check(self._lib.dymu_batch_reduce_device(
            self.ctx, dT_stack, nx, ny, B, ld, _reduce_op(op),
            None if keep is None else keep.ctypes.data, 0 if pl is None else len(pl),
            None if w is None else w.ctypes.data, None if o is None else o.ctypes.data,
            d_out or None, out_ld, d_arg or None, arg_ld, ctypes.byref(s) if summary else None,
            stream or None), self.ctx)
        return s.as_dict() if summary else None

    def last_reduce_ms(self) -> float:
        """Device time (HIP events, ms) of the last batch_reduce's kernels."""
        v = ctypes.c_double()
        _check(self._lib.dymu_last_reduce_ms(self.ctx, ctypes.byref(v)), self.ctx)
        return v.value

    def level_mask(self, d_map: int, nx: int, ny: int, ld: int, bound: float, d_mask: int,
                   mask_ld: int, region: bool = True, stream: int = 0):
        """dymu_level_mask_device: d_mask (bytes) = d_map <= bound; returns {"box": (i0, j0,
        i1, j1) inclusive, i0 > i1 when empty, "n_range": marked cells} (synchronises), or
        None with region=False (asynchronous)."""
        r = DymuRegion()
        _check(self._lib.dymu_level_mask_device(self.ctx, d_map or None, nx, ny, ld, bound,
                                                d_mask or None, mask_ld,
                                                ctypes.byref(r) if region else None,
                                                stream or None), self.ctx)
        if not region:
            return None
        return {"box": (r.i0, r.j0, r.i1, r.j1), "n_range": r.n_range, "r_const": r.r_const}

    # -- every cell's node route to the goal --
    @staticmethod
    def route_out(ld: int, sink: int = 0, axis: int = 0, diag: int = 0, length: int = 0,
                  integral=(), vmin=(), vmax=()) -> DymuRouteOut:
        """A dymu_route_out of device (or host) pointers; 0 / missing: not computed."""
        o = DymuRouteOut(sink or None, axis or None, diag or None, length or None)
        for name, ptrs in (("integral", integral), ("vmin", vmin), ("vmax", vmax)):
            arr = getattr(o, name)
            for f, q in enumerate(ptrs):
                arr[f] = q or None
        o.ld = ld
        return o

    def route_fields_workspace(self, nx: int, ny: int, n_fields: int, out=None) -> int:
        """dymu_route_fields_workspace: the bytes route_fields needs for the outputs of
        `out` (a DymuRouteOut; None: every output of n_fields fields); 0: rejected."""
        return int(self._lib.dymu_route_fields_workspace(
            nx, ny, n_fields, ctypes.byref(out) if out is not None else None))

    def route_fields(self, dT: int, nx: int, ny: int, ld: int, res: float, seeds, fields, out,
                     workspace: int, workspace_bytes: int, stream: int = 0) -> int:
        """dymu_route_fields_device on raw pointers: the routes of all cells of the device
        map dT for the seeds (i, j[, t0]) over fields, pairs (device pointer, pitch), into
        the device maps of `out` (route_out); returns the doubling rounds run.  Asynchronous
        on the stream: d2h (context stream) or last_route_fields_ms() waits for it."""
        a = self._seeds(seeds)
        fp = (_vp * max(len(fields), 1))(*[int(f[0]) for f in fields])
        fl = (_u64 * max(len(fields), 1))(*[int(f[1]) for f in fields])
        rounds = _u32()
        _check(self._lib.dymu_route_fields_device(
            self.ctx, dT, nx, ny, ld, res, a.ctypes.data, len(a), ctypes.cast(fp, _vp),
            ctypes.cast(fl, _vp), len(fields), ctypes.byref(out), workspace or None,
            workspace_bytes, stream or None, ctypes.byref(rounds)), self.ctx)
        return rounds.value

    def last_route_fields_ms(self) -> float:
        """Device time of the last route_fields, first kernel to last (waits for it)."""
        ms = ctypes.c_double()
        _check(self._lib.dymu_last_route_fields_ms(self.ctx, ctypes.byref(ms)), self.ctx)
        return ms.value

    def last_route_fields_stages(self):
        """(init, rounds, finalize) device times of the last route_fields, ms."""
        ms = (ctypes.c_double * 3)()
        _check(self._lib.dymu_last_route_fields_stages(self.ctx, ms), self.ctx)
        return tuple(ms)

    # -- how much of the map drains through every cell --
    @staticmethod
    def usage_out(ld: int, usage: int = 0, far: int = 0, sink: int = 0) -> DymuUsageOut:
        """A dymu_usage_out of device (or host) pointers; 0 / missing: not computed."""
        return DymuUsageOut(usage or None, far or None, sink or None, ld)

    def route_usage_workspace(self, nx: int, ny: int, out=None) -> int:
        """dymu_route_usage_workspace: the bytes route_usage needs for the outputs of `out`
        (a DymuUsageOut; None: every output); 0: rejected.  The catchment needs the sums:
        size a call that wants it with a non-zero usage."""
        return int(self._lib.dymu_route_usage_workspace(
            nx, ny, ctypes.byref(out) if out is not None else None))

    def route_usage(self, dT: int, nx: int, ny: int, ld: int, seeds, out, workspace: int,
                    workspace_bytes: int, weight: int = 0, weight_ld: int = 0,
                    catchment: bool = True, stream: int = 0) -> dict:
        """dymu_route_usage_device on raw pointers: usage, far and sink of all cells of the
        device map dT for the seeds (i, j[, t0]) and the device weight map (0: unit weights)
        into the device maps of `out` (usage_out).  Returns {'rounds', 'catchment'}: the
        doubling rounds run and, with catchment, one uint64 per seed (else None)."""
        a = self._seeds(seeds)
        cat = np.zeros(len(a), dtype=np.uint64) if catchment else None
        rounds = _u32()
        _check(self._lib.dymu_route_usage_device(
            self.ctx, dT, nx, ny, ld, a.ctypes.data, len(a), weight or None, weight_ld,
            ctypes.byref(out), cat.ctypes.data if catchment and len(a) else None,
            workspace or None, workspace_bytes, stream or None, ctypes.byref(rounds)), self.ctx)
        return {"rounds": rounds.value, "catchment": cat}

    def last_route_usage_ms(self) -> float:
        """Device time of the last route_usage, first kernel to last (waits for it)."""
        ms = ctypes.c_double()
        _check(self._lib.dymu_last_route_usage_ms(self.ctx, ctypes.byref(ms)), self.ctx)
        return ms.value

    def last_route_usage_stages(self):
        """(init, rounds, final) device times of the last route_usage, ms."""
        ms = (ctypes.c_double * 3)()
        _check(self._lib.dymu_last_route_usage_stages(self.ctx, ms), self.ctx)
        return tuple(ms)

    def last_route_usage_round_ms(self):
        """Device time of every round launched by the last route_usage, ms."""
        ms = (ctypes.c_double * 32)()
        n = _u32()
        _check(self._lib.dymu_last_route_usage_round_ms(self.ctx, ms, ctypes.byref(n)), self.ctx)
        return tuple(ms[:n.value])

    def alloc(self, nbytes: int) -> int:
        p = _vp()
        _check(self._lib.dymu_device_alloc(self.ctx, nbytes, ctypes.byref(p)), self.ctx)
        return p.value

    def alloc_cached(self, nbytes: int) -> int:
        """Plain (L2-cached) device memory, e.g. for a label map; free() releases it."""
        p = _vp()
        _check(self._lib.dymu_device_alloc_cached(self.ctx, nbytes, ctypes.byref(p)), self.ctx)
        return p.value

    def free(self, p: int):
        _check(self._lib.dymu_device_free(self.ctx, p), self.ctx)

    def d2h(self, dst: np.ndarray, src: int):
        _check(self._lib.dymu_memcpy_d2h(self.ctx, dst.ctypes.data, src, dst.nbytes), self.ctx)

    def h2d(self, dst: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        _check(self._lib.dymu_memcpy_h2d(self.ctx, dst, src.ctypes.data, src.nbytes), self.ctx)

    # -- row-slab domain primitives (multi-GPU sharding, dymu.sharded) --
    def dom_begin(self, F: int, T: int, nx: int, nrows: int, ld: int, ghost_lo: bool,
                  ghost_hi: bool, goal_i: int, goal_j_local: int, stream: int = 0):
        d = DymuDomain(F, T, ld, nx, nrows, int(ghost_lo), int(ghost_hi))
        self._dom = d  # keep alive
        _check(self._lib.dymu_dom_begin(self.ctx, ctypes.addressof(d), goal_i, goal_j_local,
                                        stream or None), self.ctx)

    def dom_run(self, passes: int, stream: int = 0):
        _check(self._lib.dymu_dom_run(self.ctx, passes, stream or None), self.ctx)

    def dom_merge_ghosts(self, new_lo: int = 0, new_hi: int = 0, pending: int = 0,
                         stream: int = 0):
        _check(self._lib.dymu_dom_merge_ghosts(self.ctx, new_lo or None, new_hi or None,
                                               pending or None, stream or None), self.ctx)

    def dom_exchange(self, new_lo: int = 0, new_hi: int = 0, d_total: int = 0, stream: int = 0):
        """dom_merge_ghosts with the queued-tile count in the same launch: *d_total (device
        int32, required)."""
        _check(self._lib.dymu_dom_exchange(self.ctx, new_lo or None, new_hi or None,
                                           d_total or None, stream or None), self.ctx)

    def dom_round(self, passes: int, new_lo: int = 0, new_hi: int = 0, d_total: int = 0,
                  stream: int = 0):
        """One fused round (kernel-5 domains, passes >= 2): the first pass merges the rows."""
        _check(self._lib.dymu_dom_round(self.ctx, passes, new_lo or None, new_hi or None,
                                        d_total or None, stream or None), self.ctx)

    def dom_round_supported(self, passes: int) -> int:
        return self._lib.dymu_dom_round_supported(self.ctx, passes)

    def dom_round_capable(self, nx: int, nrows: int, passes: int) -> int:
        return self._lib.dymu_dom_round_capable(self.ctx, nx, nrows, passes)

    def dom_round_peer(self, passes: int, links: "DymuPeerLinks", stream: int = 0):
        """dom_round with the peer push and the tagged merge; links: DymuPeerLinks (kept
        alive by the caller for the call only)."""
        _check(self._lib.dymu_dom_round_peer(self.ctx, passes, ctypes.addressof(links),
                                             stream or None), self.ctx)

    def dom_pending(self, stream: int = 0) -> int:
        n = ctypes.c_uint64()
        _check(self._lib.dymu_dom_pending(self.ctx, stream or None, ctypes.byref(n)), self.ctx)
        return n.value

    def set_stepping(self, on: bool = True):
        """dymu_set_stepping: the device-resident entries return after their preparation
        with the domain live; dom_run / dom_pending / dom_min_key / dom_finish drive it."""
        _check(self._lib.dymu_set_stepping(self.ctx, int(bool(on))), self.ctx)

    def dom_min_key(self, stream: int = 0) -> float:
        """dymu_dom_min_key: the smallest key of the list the next pass reads (+inf: none)."""
        k = ctypes.c_double()
        _check(self._lib.dymu_dom_min_key(self.ctx, stream or None, ctypes.byref(k)), self.ctx)
        return k.value

    def dom_snapshot(self, stream: int = 0) -> dict:
        """dymu_dom_snapshot: what the live domain starts from and carries between passes,
        as numpy arrays and plain numbers (read-only; tests and diagnostics).  eb, p, ntiles,
        tiles_cap, variant, F, T (device addresses), ld, nx, ny; tile_epoch [tiles_cap];
        counts [3, 16]; list_raw / list_tile: the entries of the list the next pass reads,
        as stored and with the key-bin field masked off.  Priority kernels: keys [3, ntiles]
        (float64), hist [3, 16, 64], minkey [3] (float64), base [3], delta; the others
        None.  ec [ntiles, 2, 16] for kernel 5 with edge columns, else None."""
        s = DymuDomState()
        _check(self._lib.dymu_dom_snapshot(self.ctx, stream or None, ctypes.addressof(s)),
               self.ctx)
        nt, keyed, ec = s.ntiles, bool(s.has_keys), bool(s.has_ec)
        out = {
            "tile_epoch": np.zeros(s.tiles_cap, dtype=np.uint32),
            "counts": np.zeros((3, 16), dtype=np.uint32),
            "list_raw": np.zeros(16 * nt, dtype=np.uint32),
            "list_tile": np.zeros(16 * nt, dtype=np.uint32),
            "keys": np.zeros((3, nt), dtype=np.uint64) if keyed else None,
            "hist": np.zeros((3, 16, 64), dtype=np.uint32) if keyed else None,
            "ec": np.zeros((nt, 2, 16)) if ec else None,
        }
        for name in out:
            if out[name] is not None:
                setattr(s, name, out[name].ctypes.data)
        s.tile_epoch_cap, s.list_cap, s.keys_cap, s.ec_cap = s.tiles_cap, 16 * nt, 3 * nt, 32 * nt
        _check(self._lib.dymu_dom_snapshot(self.ctx, stream or None, ctypes.addressof(s)),
               self.ctx)
        out["list_raw"] = out["list_raw"][:s.list_n].copy()
        out["list_tile"] = out["list_tile"][:s.list_n].copy()
        if keyed:
            out["keys"] = out["keys"].view(np.float64)
        out.update(eb=s.eb, p=s.p, ntiles=nt, tiles_cap=s.tiles_cap, variant=s.variant,
                   F=s.F or 0, T=s.T or 0, ld=s.ld, nx=s.nx, ny=s.ny,
                   minkey=np.array(s.minkey, dtype=np.uint64).view(np.float64) if keyed else None,
                   base=np.array(s.base, dtype=np.float64) if keyed else None,
                   delta=s.delta if keyed else None)
        return out

    def raise_epoch_base(self, value: int):
        """dymu_debug_raise_epoch_base: the next domain's epoch base is at least `value`
        (no domain may be live): brings the 32-bit epochs' wrap guard within reach."""
        _check(self._lib.dymu_debug_raise_epoch_base(self.ctx, int(value)), self.ctx)

    def dom_finish(self, stream: int = 0) -> dict:
        st = DymuStats()
        _check(self._lib.dymu_dom_finish(self.ctx, stream or None, ctypes.byref(st)), self.ctx)
        return st.as_dict()

    def eikonal_batch(self, tx: np.ndarray, ty: np.ndarray, c: np.ndarray,
                      fast=True) -> np.ndarray:
        """The kernels' update arithmetic on the GPU (bit-level self-test).
        fast: False = sqrt(), True = the correctly rounded sqrt in the reference's
        combine (kernels 3/4), 2 = kernel 5's default sweep candidate (monotone
        combine, approximate sqrt), 3 = kernel 5's exact_sqrt sweep candidate
        (monotone combine, correctly rounded sqrt), 4 = v31's sweep candidate."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (tx, ty, c)]
        n = arrs[0].size
        ptrs = [self.alloc(8 * n) for _ in range(4)]
        try:
            for p, a in zip(ptrs, arrs):
                self.h2d(p, a)
            _check(self._lib.dymu_eikonal_batch(self.ctx, ptrs[0], ptrs[1], ptrs[2], ptrs[3], n,
                                                fast if fast in (2, 3, 4) else 1 if fast else 0),
                   self.ctx)
            out = np.empty(n)
            self.d2h(out, ptrs[3])
            return out
        finally:
            for p in ptrs:
                self.free(p)

    def pass_scan_probe(self, counts, hist, target: int, target_frac: float = 0.0,
                        cap_frac: float = 0.0):
        """dymu_pass_scan_probe: the priority passes' list scan on 16 shard counts and a
        16 x 64 key histogram.  Returns (prefix[0..16] as uint32, b*)."""
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        hist = np.ascontiguousarray(hist, dtype=np.uint32)
        if counts.shape != (16,) or hist.shape != (16, 64):
            raise ValueError("counts: 16 words, hist: 16 x 64 words")
        prefix = np.empty(17, dtype=np.uint32)
        bstar = ctypes.c_int32()
        _check(self._lib.dymu_pass_scan_probe(self.ctx, counts.ctypes.data, hist.ctypes.data,
                                              target, target_frac, cap_frac, prefix.ctypes.data,
                                              ctypes.byref(bstar)), self.ctx)
        return prefix, bstar.value

    # ---- computeCostMap on the device ----
    @staticmethod
    def cost_state(ptrs: dict) -> DymuCostState:
        """ptrs: field name -> device pointer (int), see DymuCostState.FIELDS."""
        return DymuCostState(*[ptrs[f] for f in DymuCostState.FIELDS])

    def compute_cost_map(self, nx, ny, ld, res, lut, slopes, n_locs, d_elev, d_terrain,
                         state: dict, dF=0, stream=0):
        lut = np.ascontiguousarray(lut, dtype=np.float64)
        slopes = np.ascontiguousarray(slopes, dtype=np.float64)
        st = self.cost_state(state)
        _check(self._lib.dymu_compute_cost_map(self.ctx, nx, ny, ld, res, lut, len(lut), slopes,
                                               len(slopes), n_locs, d_elev, d_terrain,
                                               ctypes.byref(st), dF or None, stream or None),
               self.ctx)

    def pack_speed(self, nx, ny, ld, res, state: dict, dF, stream=0):
        st = self.cost_state(state)
        _check(self._lib.dymu_pack_speed(self.ctx, nx, ny, ld, res, ctypes.byref(st), dF,
                                         stream or None), self.ctx)

    def set_profiling(self, period):
        """Time every `period`-th pass launch (True = every launch, 0/False = off)."""
        _check(self._lib.dymu_set_profiling(self.ctx, int(period)), self.ctx)

    PASS_STAT_FIELDS = ("listed", "visited", "colour_deferred", "key_deferred", "capped",
                        "deadline", "radius_max", "sweeps", "bstar", "radius_min", "enqueued")

    def last_update_stats(self) -> dict:
        """The last windowed update's raise front (dymu_last_update_stats)."""
        out = (_u64 * 4)()
        _check(self._lib.dymu_last_update_stats(self.ctx, out), self.ctx)
        return {"raise_passes": out[0], "raise_visits": out[1], "cells_invalidated": out[2]}

    def set_pass_stats(self, on=True):
        """Kernel 5 per-pass statistics for the next solves (diagnostics)."""
        _check(self._lib.dymu_set_pass_stats(self.ctx, int(bool(on))), self.ctx)

    def last_pass_stats(self) -> np.ndarray:
        """(passes, 12) uint32 records of the last solve (fields: PASS_STAT_FIELDS)."""
        n = _u64()
        cap = 1 << 14
        out = np.zeros((cap, 12), dtype=np.uint32)
        _check(self._lib.dymu_last_pass_stats(self.ctx, out.ctypes.data, cap, ctypes.byref(n)),
               self.ctx)
        return out[:n.value].copy()

    def last_pass_timing(self):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        _check(self._lib.dymu_last_pass_timing(self.ctx, ctypes.byref(ms), ctypes.byref(n)),
               self.ctx)
        return ms.value, n.value


def slab_rows(ny: int, nranks: int, rank: int):
    """(row0, nrows) of `rank`'s row slab (boundaries on multiples of 32 rows)."""
    r0, n = ctypes.c_uint32(), ctypes.c_uint32()
    _check(load_fim().dymu_slab_rows(ny, nranks, rank, ctypes.byref(r0), ctypes.byref(n)))
    return r0.value, n.value


def batch_plane_rows(ny: int) -> int:
    """The plane pitch in rows of a batch of ny-row maps: 16 * ceil((ny + 1) / 16)."""
    return int(load_fim().dymu_batch_plane_rows(ny))


def device_count() -> int:
    return load_fim().dymu_device_count()


# ---------------------------------------------------------------------------
# host planner: PathPlanning_lib::DyMuPathPlanner behind include/dymu_planner.h
# ---------------------------------------------------------------------------
_d = ctypes.c_double
PLANNER_SYMBOLS = {
    "dymu_planner_create": (_i32, [ctypes.POINTER(_vp), _d, _d, _d, _i32]),
    "dymu_planner_destroy": (None, [_vp]),
    "dymu_planner_set_engine_options": (_i32, [_vp, ctypes.POINTER(DymuOpts)]),
    "dymu_planner_init_global_layer": (_i32, [_vp, _d, _d, _u32, _u32, _d, _d]),
    "dymu_planner_set_cost_map": (_i32, [_vp, _dp, _u32, _u32]),
    "dymu_planner_compute_cost_map": (_i32, [_vp, _dp, _i32, _dp, _i32,
                                             ctypes.POINTER(ctypes.c_char_p), _i32, _dp, _dp]),
    "dymu_planner_set_goal": (_i32, [_vp, _d, _d, _d, _d]),
    "dymu_planner_compute_total_cost_map": (_i32, [_vp, _d, _d, _d, _d]),
    "dymu_planner_compute_entire_total_cost_map": (_i32, [_vp]),
    "dymu_planner_get_total_cost_matrix": (_i32, [_vp, _dp]),
    "dymu_planner_get_global_cost_matrix": (_i32, [_vp, _dp]),
    "dymu_planner_get_hazard_density_matrix": (_i32, [_vp, _dp]),
    "dymu_planner_get_trafficability_matrix": (_i32, [_vp, _dp]),
    "dymu_planner_get_total_cost_raw": (_i32, [_vp, _dp]),
    "dymu_planner_get_total_cost": (_i32, [_vp, _d, _d, _d, _d, ctypes.POINTER(_d)]),
    "dymu_planner_get_path": (_i32, [_vp, _d, _d, _d, _d, _dp, _i32]),
    "dymu_planner_get_paths": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "dymu_planner_set_goals": (_i32, [_vp, _vp, _vp, _i32]),
    "dymu_planner_goal_count": (_i32, [_vp]),
    "dymu_planner_get_goal_labels": (_i32, [_vp, _vp]),
    "dymu_planner_goal_label": (_i32, [_vp, _d, _d]),
    "dymu_planner_last_path_sinks": (_i32, [_vp, _vp, _i32]),
    "dymu_planner_last_paths_on_device": (_i32, [_vp]),
    "dymu_planner_last_paths_kernel_ms": (_i32, [_vp, ctypes.POINTER(_d)]),
    "dymu_planner_compute_total_cost_maps": (_i32, [_vp, _vp, _i32]),
    "dymu_planner_batch_count": (_i32, [_vp]),
    "dymu_planner_copy_batch_total_cost": (_i32, [_vp, _u32, _dp, _i32]),
    "dymu_planner_get_total_costs": (_i32, [_vp, _vp, _i32, _vp]),
    "dymu_planner_cost_matrix": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp]),
    "dymu_planner_cost_matrix_until": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp]),
    "dymu_planner_batch_level": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_planner_get_paths_to": (_i32, [_vp, _u32, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "dymu_planner_last_batch_stats": (_i32, [_vp, ctypes.POINTER(DymuStats)]),
    "dymu_planner_track_speed_changes": (_i32, [_vp, _i32]),
    "dymu_planner_last_batch_solve_kind": (_i32, [_vp]),
    "dymu_planner_combine_total_cost_maps": (_i32, [_vp, _i32, _vp, _u32, _vp, _vp,
                                                    ctypes.POINTER(DymuReduceSummary)]),
    "dymu_planner_copy_combined_total_cost": (_i32, [_vp, _vp, _i32]),
    "dymu_planner_copy_combined_planes": (_i32, [_vp, _vp]),
    "dymu_planner_via_corridor": (_i32, [_vp, _u32, _u32, ctypes.c_double, _vp,
                                         ctypes.POINTER(DymuCorridorInfo)]),
    "dymu_planner_rendezvous": (_i32, [_vp, _vp, _u32, _vp, _vp, _i32, ctypes.POINTER(_u32),
                                       ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_double)]),
    "dymu_planner_last_combine_kernel_ms": (_i32, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "dymu_planner_get_path_stats": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "dymu_planner_get_path_stats_to": (_i32, [_vp, _u32, _vp, _i32, _i32, _vp, _vp]),
    "dymu_planner_get_arriving_paths": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "dymu_planner_get_arriving_paths_to": (_i32, [_vp, _u32, _vp, _i32, _i32, _i32, _vp, _vp, _vp,
                                                  _vp]),
    "dymu_planner_get_simplified_paths": (_i32, [_vp, _vp, _i32, ctypes.c_double, _i32, _vp, _vp,
                                                 _vp, _vp, _vp]),
    "dymu_planner_get_simplified_paths_to": (_i32, [_vp, _u32, _vp, _i32, ctypes.c_double, _i32,
                                                    _vp, _vp, _vp, _vp, _vp]),
    "dymu_planner_last_simplified": (_i32, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "dymu_planner_get_arriving_stats": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "dymu_planner_get_arriving_stats_to": (_i32, [_vp, _u32, _vp, _i32, _i32, _vp]),
    "dymu_planner_get_route_fields": (_i32, [_vp, _vp, _i32, _i32, ctypes.POINTER(DymuRouteOut),
                                             ctypes.POINTER(_u32)]),
    "dymu_planner_get_route_fields_to": (_i32, [_vp, _u32, _vp, _i32,
                                                ctypes.POINTER(DymuRouteOut),
                                                ctypes.POINTER(_u32)]),
    "dymu_planner_get_route_usage": (_i32, [_vp, _vp, _i32, ctypes.POINTER(DymuUsageOut), _vp,
                                            _u32, ctypes.POINTER(_u32)]),
    "dymu_planner_get_route_usage_to": (_i32, [_vp, _u32, _vp, ctypes.POINTER(DymuUsageOut), _vp,
                                               _u32, ctypes.POINTER(_u32)]),
    "dymu_planner_goal_cell": (_i32, [_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "dymu_planner_get_locomotion_mode": (_i32, [_vp, _d, _d, _d, _d, ctypes.c_char_p, _i32]),
    "dymu_planner_set_global_risk": (_i32, [_vp, _d, _d]),
    "dymu_planner_get_global_risk": (_i32, [_vp, _dp]),
    "dymu_planner_set_hazard_density": (_i32, [_vp, _dp]),
    "dymu_planner_set_trafficability": (_i32, [_vp, _dp]),
    "dymu_planner_last_stats": (_i32, [_vp, ctypes.POINTER(DymuStats)]),
    "dymu_planner_last_solve_kind": (_i32, [_vp]),
    "dymu_planner_last_early_exit": (_i32, [_vp, _dp]),
    "dymu_planner_last_early_exit_ex": (_i32, [_vp, _vp, _u32]),
    "dymu_planner_get_node_states": (_i32, [_vp, _vp]),
    "dymu_planner_set_hazard_density_window": (_i32, [_vp, _u32, _u32, _u32, _u32, _dp]),
    "dymu_planner_set_trafficability_window": (_i32, [_vp, _u32, _u32, _u32, _u32, _dp]),
    "dymu_planner_set_cost_map_window": (_i32, [_vp, _u32, _u32, _u32, _u32, _dp]),
    "dymu_planner_last_risk_update_kind": (_i32, [_vp]),
    "dymu_planner_track_obstacle_removal": (_i32, [_vp, _i32]),
    "dymu_planner_last_risk_raise": (_i32, [_vp, ctypes.POINTER(_u64)]),
    "dymu_planner_last_risk_update": (_i32, [_vp, ctypes.POINTER(DymuStats),
                                             ctypes.POINTER(_u32)]),
    "dymu_planner_last_band_size": (ctypes.c_int64, [_vp]),
    "dymu_planner_get_global_node": (_i32, [_vp, _u32, _u32, _vp]),
    "dymu_planner_is_safe_node": (_i32, [_vp, _u32, _u32]),
    "dymu_planner_is_fully_closed_node": (_i32, [_vp, _u32, _u32]),
    "dymu_planner_global_narrowband": (ctypes.c_int64, [_vp, _vp, ctypes.c_int64]),
    "dymu_planner_min_cost_global_node": (_i32, [_vp, _vp, _dp]),
    "dymu_planner_reset_global_narrow_band": (_i32, [_vp]),
    "dymu_planner_gradient_node": (_i32, [_vp, _u32, _u32, _dp]),
    "dymu_planner_local_waypoint_dijkstra": (_i32, [_vp, _dp, _dp]),
    "dymu_planner_local_agent": (_i32, [_vp, _dp]),
    "dymu_planner_reset_total_cost_map": (_i32, [_vp]),
    "dymu_planner_load_total_cost_map": (_i32, [_vp, _dp]),
    "dymu_planner_set_current_path": (_i32, [_vp, _vp, _i32]),
    "dymu_planner_get_current_path": (_i32, [_vp, _dp, _i32]),
    "dymu_planner_compute_local_planning": (_i32, [_vp, _d, _d, _d, _d, _vp, _u32, _u32, _u32,
                                                   _u32, _d, _dp, _i32, ctypes.POINTER(_i32),
                                                   ctypes.POINTER(_d)]),
    "dymu_planner_repair_path": (_i32, [_vp, _d, _d, _d, _d, _u32]),
    "dymu_planner_evaluate_path": (_i32, [_vp, _u32]),
    "dymu_planner_expand_risk": (_i32, [_vp]),
    "dymu_planner_compute_local_propagation": (_i32, [_vp, _dp, _dp, _dp]),
    "dymu_planner_set_local_timeout": (_i32, [_vp, ctypes.c_double]),
    "dymu_planner_get_risk_matrix": (_i32, [_vp, _d, _d, _d, _d, _dp]),
    "dymu_planner_get_deviation_matrix": (_i32, [_vp, _d, _d, _d, _d, _dp]),
    "dymu_planner_get_reconnecting_index": (_i32, [_vp]),
    "dymu_planner_res_ratio": (_i32, [_vp]),
    "dymu_planner_local_map_mask": (ctypes.c_int64, [_vp, _vp]),
    "dymu_planner_local_block": (_i32, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "dymu_planner_propagate_global_node": (_i32, [_vp, _u32, _u32]),
    "dymu_planner_set_global_node_state": (_i32, [_vp, _u32, _u32, _i32]),
    "dymu_planner_global_propagated_nodes": (ctypes.c_int64, [_vp, _vp, ctypes.c_int64]),
    "dymu_planner_get_local_node": (_i32, [_vp, _d, _d, _vp]),
    "dymu_planner_max_risk_node": (_i32, [_vp, _vp]),
    "dymu_planner_local_neighbour": (_i32, [_vp, _u64, _i32, _vp]),
    "dymu_planner_propagate_risk": (_i32, [_vp, _u64]),
    "dymu_planner_propagate_local_node": (_i32, [_vp, _u64]),
    "dymu_planner_set_local_node_state": (_i32, [_vp, _u64, _i32]),
    "dymu_planner_min_cost_local_node": (_i32, [_vp, _d, _d, _vp]),
    "dymu_planner_min_cost_local_node_reach": (_i32, [_vp, _u64, _vp]),
    "dymu_planner_local_list": (ctypes.c_int64, [_vp, _i32, _vp, ctypes.c_int64]),
}


class DymuGlobalNode(ctypes.Structure):
    _fields_ = [("elevation", _d), ("slope", _d), ("raw_cost", _d), ("cost", _d),
                ("hazard_density", _d), ("trafficability", _d), ("total_cost", _d),
                ("terrain", _u32), ("state", _i32), ("is_obstacle", _i32),
                ("has_local_map", _i32)]

class DymuLocalNode(ctypes.Structure):
    _fields_ = [("global_x", _d), ("global_y", _d), ("deviation", _d), ("total_cost", _d),
                ("risk", _d), ("parent_i", _u32), ("parent_j", _u32), ("li", _u32),
                ("lj", _u32), ("state", _i32), ("is_obstacle", _i32), ("id", _u64)]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


_pl = None


def load_planner() -> ctypes.CDLL:
    global _pl
    if _pl is None:
        load_fim()
        path = lib_path("libdymu_planner.so")
        if not os.path.exists(path):
            raise DymuError(-5, f"planner library missing: {path} (run __graft_entry__.build())")
        lib = ctypes.CDLL(path)
        ab_build = "DYMU_LIBDIR" in os.environ  # an older A/B build may lack newer symbols
        for name, (res, args) in PLANNER_SYMBOLS.items():
            if ab_build and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _pl = lib
    return _pl


def _b_int(rc: int) -> int:
    if rc < 0:
        raise DymuError(rc)
    return rc


def _b(rc: int) -> bool:
    if rc < 0:
        raise DymuError(rc)
    return bool(rc)


class Planner:
    """Python mirror of PathPlanning_lib::DyMuPathPlanner (reference
    src/DyMu.hpp:397-609, global layer).  Method names follow the reference;
    waypoints are (x, y[, z, heading]) tuples; grids are numpy [ny, nx]."""

    CONSERVATIVE, SWEEPING = 0, 1

    def __init__(self, risk_distance=1.0, reconnect_distance=1.0, risk_ratio=1.0,
                 approach=CONSERVATIVE, device: int = -1):
        self._lib = load_planner()
        h = _vp()
        rc = self._lib.dymu_planner_create(ctypes.byref(h), risk_distance, reconnect_distance,
                                           risk_ratio, approach)
        if rc != DYMU_OK:
            raise DymuError(rc, "dymu_planner_create")
        self.h = h
        self.nx = self.ny = 0
        self._sinks = np.zeros(0, dtype=np.int32)
        if device >= 0:
            o = DymuOpts(device, 0, 0, 0, 0)
            _check(self._lib.dymu_planner_set_engine_options(self.h, ctypes.byref(o)))

    def close(self):
        if getattr(self, "h", None):
            self._lib.dymu_planner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _wp(w):
        w = tuple(w) + (0.0,) * (4 - len(w))
        return float(w[0]), float(w[1]), float(w[2]), float(w[3])

    def _grid(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (self.ny, self.nx):
            raise ValueError(f"expected [{self.ny}, {self.nx}] grid, got {a.shape}")
        return a

    def initGlobalLayer(self, globalres, localres, nx, ny, offset=(0.0, 0.0)) -> bool:
        self.nx, self.ny = int(nx), int(ny)
        return _b(self._lib.dymu_planner_init_global_layer(self.h, globalres, localres, nx, ny,
                                                           offset[0], offset[1]))

    def setCostMap(self, cost_map) -> bool:
        a = np.ascontiguousarray(cost_map, dtype=np.float64)
        ny, nx = a.shape
        return _b(self._lib.dymu_planner_set_cost_map(self.h, a, nx, ny))

    def computeCostMap(self, cost_data, slope_values, locomotion_modes, elevation,
                       terrain_map) -> bool:
        lut = np.ascontiguousarray(cost_data, dtype=np.float64)
        sl = np.ascontiguousarray(slope_values, dtype=np.float64)
        modes = (ctypes.c_char_p * len(locomotion_modes))(*[m.encode() for m in locomotion_modes])
        return _b(self._lib.dymu_planner_compute_cost_map(
            self.h, lut, len(lut), sl, len(sl), modes, len(locomotion_modes),
            self._grid(elevation), self._grid(terrain_map)))

    def setGoal(self, w) -> bool:
        return _b(self._lib.dymu_planner_set_goal(self.h, *self._wp(w)))

    def setGoals(self, goals, offsets=None) -> bool:
        """DyMuPathPlanner::setGoals: several goals (x, y[, z, heading]) at once, each with
        an optional offset >= 0.  False (and nothing changed) if any is rejected."""
        g = np.ascontiguousarray([self._wp(w) for w in goals], dtype=np.float64).reshape(-1, 4)
        off = None
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.float64).ravel()
            if len(off) != len(g):
                return False
        if len(g) == 0:
            return False
        return _b(self._lib.dymu_planner_set_goals(
            self.h, g.ctypes.data, None if off is None else off.ctypes.data, len(g)))

    def goalCount(self) -> int:
        return _b_int(self._lib.dymu_planner_goal_count(self.h))

    def goalLabels(self) -> np.ndarray:
        """The nearest-goal label of every node, [ny, nx] uint32 (LABEL_NONE: none)."""
        out = np.empty((self.ny, self.nx), dtype=np.uint32)
        _check(self._lib.dymu_planner_get_goal_labels(self.h, out.ctypes.data))
        return out

    def goalLabel(self, w) -> int:
        """The label of the node nearest w, -1 for none."""
        x, y, _, _ = self._wp(w)
        rc = self._lib.dymu_planner_goal_label(self.h, x, y)
        if rc < -1:
            raise DymuError(rc)
        return rc

    def lastPathSinks(self) -> np.ndarray:
        """The goal each path of the last getPaths ended on (-1 where status != 1)."""
        return self._sinks.copy()

    def computeTotalCostMap(self, w) -> bool:
        return _b(self._lib.dymu_planner_compute_total_cost_map(self.h, *self._wp(w)))

    def computeEntireTotalCostMap(self) -> bool:
        return _b(self._lib.dymu_planner_compute_entire_total_cost_map(self.h))

    def _matrix(self, fn):
        out = np.empty((self.ny, self.nx))
        _check(fn(self.h, out))
        return out

    def getTotalCostMatrix(self):
        return self._matrix(self._lib.dymu_planner_get_total_cost_matrix)

    def getGlobalCostMatrix(self):
        return self._matrix(self._lib.dymu_planner_get_global_cost_matrix)

    def getHazardDensityMatrix(self):
        return self._matrix(self._lib.dymu_planner_get_hazard_density_matrix)

    def getTrafficabilityMatrix(self):
        return self._matrix(self._lib.dymu_planner_get_trafficability_matrix)

    def totalCostRaw(self):
        return self._matrix(self._lib.dymu_planner_get_total_cost_raw)

    def getTotalCost(self, w) -> float:
        out = ctypes.c_double()
        _check(self._lib.dymu_planner_get_total_cost(self.h, *self._wp(w), ctypes.byref(out)))
        return out.value

    def getPath(self, w, max_wp: int = 1 << 20) -> np.ndarray:
        buf = np.empty(4 * max_wp)
        n = self._lib.dymu_planner_get_path(self.h, *self._wp(w), buf, max_wp)
        if n < 0:
            raise DymuError(n)
        return buf[:4 * min(n, max_wp)].reshape(-1, 4).copy()

    def getPaths(self, starts, max_wp: int = 1 << 20, stride: int = 1):
        """Batched getPath without evaluatePath (DyMuPathPlanner::getPaths): the global
        path of every start (x, y[, z, heading]) on the current map, on the GPU while the
        device map is current.  Returns (list of (n_q, 4) arrays, status int32 array: 1
        sink appended, 0 stalled, -1 first step NaN / off the grid, -3 max_wp reached).
        current_path is not touched."""
        s = np.ascontiguousarray([self._wp(w) for w in starts], dtype=np.float64).reshape(-1, 4)
        n = len(s)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        st = np.zeros(max(n, 1), dtype=np.int32)
        _b_int(self._lib.dymu_planner_get_paths(self.h, s.ctypes.data, n, max_wp, stride, None,
                                                cnt.ctypes.data, st.ctypes.data))
        self._sinks = np.full(n, -1, dtype=np.int32)
        if n:
            _b_int(self._lib.dymu_planner_last_path_sinks(self.h, self._sinks.ctypes.data, n))
        buf = np.empty((max(int(cnt[:n].sum()), 1), 4))
        _b_int(self._lib.dymu_planner_get_paths(self.h, None, n, 0, 0, buf.ctypes.data, None,
                                                None))
        ends = np.cumsum(cnt[:n])
        return [buf[e - c:e].copy() for e, c in zip(ends, cnt[:n])], st[:n].copy()

    # -- batched total-cost maps (DyMuPathPlanner::computeTotalCostMaps) --
    def computeTotalCostMaps(self, goals) -> bool:
        """One total-cost map per goal (x, y[, z, heading]) on the current speed, solved
        together and kept on the device next to the single goal's map.  False (nothing
        changed) if a goal is rejected or there is no device engine."""
        g = np.ascontiguousarray([self._wp(w) for w in goals], dtype=np.float64).reshape(-1, 4)
        if len(g) == 0:
            return False
        return _b(self._lib.dymu_planner_compute_total_cost_maps(self.h, g.ctypes.data, len(g)))

    def batchCount(self) -> int:
        return _b_int(self._lib.dymu_planner_batch_count(self.h))

    def batchTotalCost(self, b: int, raw: bool = True):
        """Map b of the batch, [ny, nx] (+inf unreachable; raw=False: -1), or None."""
        out = np.empty((self.ny, self.nx))
        if b < 0 or not _b(self._lib.dymu_planner_copy_batch_total_cost(self.h, b, out, int(raw))):
            return None
        return out

    # -- combining the maps of the batch --
    def _combine_lists(self, planes, weights, offsets):
        """The lists as arrays (None stays None), or False where their lengths do not fit."""
        pl = None if planes is None else np.ascontiguousarray(planes, dtype=np.int64).ravel()
        n = self.batchCount() if pl is None else len(pl)
        if n == 0 or (pl is not None and ((pl < 0) | (pl > 0xFFFFFFFF)).any()):
            return False
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).ravel()
        o = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64).ravel()
        if any(a is not None and len(a) != n for a in (w, o)):
            return False
        return (None if pl is None else pl.astype(np.uint32)), w, o, n

    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data

    def combineTotalCostMaps(self, op, planes=None, weights=None, offsets=None):
        """The maps of the batch combined cell by cell on the device: op ("sum" / "max" /
        "min" or 0 / 1 / 2) over the listed maps (None: all), each optionally weighted and
        offset.  Returns the summary of the combined map as a dict (min_value, min_i, min_j,
        min_plane, n_finite), or False (nothing changed) without a batch or a device engine
        and for a bad list."""
        l = self._combine_lists(planes, weights, offsets)
        if l is False:
            return False
        pl, w, o, n = l
        s = DymuReduceSummary()
        if not _b(self._lib.dymu_planner_combine_total_cost_maps(
                self.h, _reduce_op(op), self._ptr(pl), n if pl is not None else 0, self._ptr(w),
                self._ptr(o), ctypes.byref(s))):
            return False
        return s.as_dict()

    def _out(self, out, dtype):
        """A caller's C-contiguous [ny, nx] array of dtype to fill, or a fresh one."""
        if out is None:
            return np.empty((self.ny, self.nx), dtype=dtype)
        if out.shape != (self.ny, self.nx) or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError(f"expected a C-contiguous [{self.ny}, {self.nx}] {dtype} array")
        return out

    def combinedTotalCost(self, raw: bool = True, out=None):
        """The combined map, [ny, nx] (+inf; raw=False: -1), or False once it no longer
        belongs to the held batch.  out: an array to fill instead of a new one."""
        out = self._out(out, np.float64)
        if not _b(self._lib.dymu_planner_copy_combined_total_cost(self.h, out.ctypes.data,
                                                                  int(raw))):
            return False
        return out

    def combinedPlanes(self, out=None):
        """The plane that gave each cell of the last MAX / MIN, [ny, nx] uint32 (LABEL_NONE:
        a MIN cell no plane reaches), or False.  out: an array to fill instead of a new one."""
        out = self._out(out, np.uint32)
        if not _b(self._lib.dymu_planner_copy_combined_planes(self.h, out.ctypes.data)):
            return False
        return out

    def viaCorridor(self, a: int, b: int, slack: float, mask=None):
        """(mask [ny, nx] uint8, info dict) of the corridor between goals a and b: the cells
        whose via cost T_a + T_b is within (1 + slack) of its minimum D_min; or False (a
        caller's mask is then left as it was)."""
        if a < 0 or b < 0 or a > 0xFFFFFFFF or b > 0xFFFFFFFF:
            return False
        mask = self._out(mask, np.uint8)
        ci = DymuCorridorInfo()
        if not _b(self._lib.dymu_planner_via_corridor(self.h, a, b, float(slack), mask.ctypes.data,
                                                      ctypes.byref(ci))):
            return False
        return mask, {"D_min": ci.d_min, "cell": (ci.min_i, ci.min_j), "count": ci.count,
                      "box": (ci.i0, ci.j0, ci.i1, ci.j1), "bound": ci.bound}

    def rendezvous(self, planes=None, weights=None, offsets=None, minimax: bool = True):
        """(i, j, value): the cell minimising the MAX (minimax) or the SUM of the listed maps,
        the lowest row-major one among equals; False when there is none."""
        l = self._combine_lists(planes, weights, offsets)
        if l is False:
            return False
        pl, w, o, n = l
        i, j, v = _u32(), _u32(), ctypes.c_double()
        if not _b(self._lib.dymu_planner_rendezvous(
                self.h, self._ptr(pl), n if pl is not None else 0, self._ptr(w), self._ptr(o),
                int(bool(minimax)), ctypes.byref(i), ctypes.byref(j), ctypes.byref(v))):
            return False
        return i.value, j.value, v.value

    def lastCombineKernelMs(self) -> float:
        v = ctypes.c_double()
        _check(self._lib.dymu_planner_last_combine_kernel_ms(self.h, ctypes.byref(v)))
        return v.value

    @staticmethod
    def _xy(points) -> np.ndarray:
        return np.ascontiguousarray([(float(w[0]), float(w[1])) for w in points],
                                    dtype=np.float64).reshape(-1, 2)

    def getTotalCosts(self, points):
        """[batchCount, len(points)]: getTotalCost of every point on every map of the batch
        (evaluated on the device), or None without a batch."""
        xy = self._xy(points)
        out = np.zeros((self.batchCount(), len(xy)))
        if not _b(self._lib.dymu_planner_get_total_costs(self.h, xy.ctypes.data, len(xy),
                                                         out.ctypes.data)):
            return None
        return out

    def costMatrix(self, goals, targets, until: bool = False):
        """computeTotalCostMaps(goals) and getTotalCosts(targets) in one call: the
        [len(goals), len(targets)] traverse-cost matrix, or None on failure.  until=True
        (costMatrixUntil): the batch solve stops once the cells the targets
        read are final in every map -- the same matrix, and a truncated batch (batchLevel()
        finite) that the batch readers complete with a cold solve before they use it."""
        g = np.ascontiguousarray([self._wp(w) for w in goals], dtype=np.float64).reshape(-1, 4)
        xy = self._xy(targets)
        if len(g) == 0:
            return None
        out = np.zeros((len(g), len(xy)))
        fn = self._lib.dymu_planner_cost_matrix_until if until else \
            self._lib.dymu_planner_cost_matrix
        if not _b(fn(self.h, g.ctypes.data, len(g), xy.ctypes.data, len(xy), out.ctypes.data)):
            return None
        return out

    def batchLevel(self) -> float:
        """The level up to which the held batch's maps are final: finite after
        costMatrix(..., until=True), +inf for a complete batch and with no batch."""
        v = ctypes.c_double()
        _check(self._lib.dymu_planner_batch_level(self.h, ctypes.byref(v)))
        return v.value

    def getPathsTo(self, b: int, starts, max_wp: int = 1 << 20, stride: int = 1):
        """getPaths on map b of the batch, with goal b as the sink: (paths, status)."""
        s = np.ascontiguousarray([self._wp(w) for w in starts], dtype=np.float64).reshape(-1, 4)
        n = len(s)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        st = np.zeros(max(n, 1), dtype=np.int32)
        _b_int(self._lib.dymu_planner_get_paths_to(self.h, b, s.ctypes.data, n, max_wp, stride,
                                                   None, cnt.ctypes.data, st.ctypes.data))
        buf = np.empty((max(int(cnt[:n].sum()), 1), 4))
        _b_int(self._lib.dymu_planner_get_paths_to(self.h, b, None, n, 0, 0, buf.ctypes.data,
                                                   None, None))
        ends = np.cumsum(cnt[:n])
        return [buf[e - c:e].copy() for e, c in zip(ends, cnt[:n])], st[:n].copy()

    def _stats_args(self, starts, field):
        s = np.ascontiguousarray([self._wp(w) for w in starts], dtype=np.float64).reshape(-1, 4)
        f = None if field is None else self._grid(field)
        out = np.zeros(len(s), dtype=PATH_STAT_DTYPE)
        return s, f, out

    def getPathStats(self, starts, max_wp: int = 1 << 20, field=None, host: bool = False):
        """One record per start instead of its path (DyMuPathPlanner::getPathStats, DESIGN.md
        s5.13): a PATH_STAT_DTYPE array with getPaths' status / sink / count, the length, the
        last hop (<= (2 + tau) res where the descent arrived; longer where it was cut short
        and jumped to the sink), and per field the integral along the path, min, max and
        skipped samples -- slot 0 the speed map the solve used, slot 1 the optional [ny, nx]
        `field`.  On the GPU while the device map is current (no waypoint is stored or
        moved), else -- or with host=True -- on the host threads, bit-identically."""
        s, f, out = self._stats_args(starts, field)
        _b_int(self._lib.dymu_planner_get_path_stats(
            self.h, s.ctypes.data, len(s), max_wp, None if f is None else f.ctypes.data,
            int(bool(host)), out.ctypes.data))
        return out

    def getPathStatsTo(self, b: int, starts, max_wp: int = 1 << 20, field=None):
        """getPathStats on map b of the batch, with goal b as the sink."""
        s, f, out = self._stats_args(starts, field)
        _b_int(self._lib.dymu_planner_get_path_stats_to(
            self.h, b, s.ctypes.data, len(s), max_wp, None if f is None else f.ctypes.data,
            out.ctypes.data))
        return out

    # -- the arriving descent (DyMuPathPlanner::getArrivingPaths) --
    def _arriving(self, fn, pre, starts, max_wp, stride):
        s = np.ascontiguousarray([self._wp(w) for w in starts], dtype=np.float64).reshape(-1, 4)
        n = len(s)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        st = np.zeros(max(n, 1), dtype=np.int32)
        rec = np.zeros(max(n, 1), dtype=ARRIVE_STAT_DTYPE)
        _b_int(fn(self.h, *pre, s.ctypes.data, n, max_wp, stride, None, cnt.ctypes.data,
                  st.ctypes.data, rec.ctypes.data))
        self._sinks = np.full(n, -1, dtype=np.int32)
        if n:
            _b_int(self._lib.dymu_planner_last_path_sinks(self.h, self._sinks.ctypes.data, n))
        buf = np.empty((max(int(cnt[:n].sum()), 1), 4))
        _b_int(fn(self.h, *pre, None, n, 0, 0, buf.ctypes.data, None, None, None))
        ends = np.cumsum(cnt[:n])
        return ([buf[e - c:e].copy() for e, c in zip(ends, cnt[:n])], st[:n].copy(),
                rec[:n].copy())

    def getArrivingPaths(self, starts, max_wp: int = 1 << 20, stride: int = 1):
        """getPaths with the arriving descent: paths that pass obstacles and end on the
        goal's node -- the continuous descent wherever it is valid, a node-to-node step on
        the total cost wherever it is not, never inside an obstacle node's square.  Returns
        (paths, status, records): getPaths' two, and an ARRIVE_STAT_DTYPE array (status,
        sink, waypoints and hops at stride 1, length, total cost at the start's node).
        Status -1: the start's node is off the grid, an obstacle or without a label.
        lastPathSinks / lastPathsOnDevice / lastPathsKernelMs report the call."""
        return self._arriving(self._lib.dymu_planner_get_arriving_paths, (), starts, max_wp,
                              stride)

    def getArrivingPathsTo(self, b: int, starts, max_wp: int = 1 << 20, stride: int = 1):
        """getArrivingPaths on map b of the batch, with goal b as the sink."""
        return self._arriving(self._lib.dymu_planner_get_arriving_paths_to, (b,), starts, max_wp,
                              stride)

    def getArrivingStats(self, starts, max_wp: int = 1 << 20, host: bool = False):
        """The records of getArrivingPaths alone: no waypoint is stored or moved."""
        s = np.ascontiguousarray([self._wp(w) for w in starts], dtype=np.float64).reshape(-1, 4)
        out = np.zeros(len(s), dtype=ARRIVE_STAT_DTYPE)
        _b_int(self._lib.dymu_planner_get_arriving_stats(self.h, s.ctypes.data, len(s), max_wp,
                                                         int(bool(host)), out.ctypes.data))
        return out

    def getArrivingStatsTo(self, b: int, starts, max_wp: int = 1 << 20):
        """getArrivingStats on map b of the batch, with goal b as the sink."""
        s = np.ascontiguousarray([self._wp(w) for w in starts], dtype=np.float64).reshape(-1, 4)
        out = np.zeros(len(s), dtype=ARRIVE_STAT_DTYPE)
        _b_int(self._lib.dymu_planner_get_arriving_stats_to(self.h, b, s.ctypes.data, len(s),
                                                            max_wp, out.ctypes.data))
        return out

    # -- arriving paths thinned within a bound (DyMuPathPlanner::getSimplifiedPaths, s5.18) --
    def _simplified(self, fn, pre, starts, eps, max_wp):
        s = np.ascontiguousarray([self._wp(w) for w in starts], dtype=np.float64).reshape(-1, 4)
        n = len(s)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        st = np.zeros(max(n, 1), dtype=np.int32)
        rec = np.zeros(max(n, 1), dtype=ARRIVE_STAT_DTYPE)
        _b_int(fn(self.h, *pre, s.ctypes.data, n, eps, max_wp, None, None, cnt.ctypes.data,
                  st.ctypes.data, rec.ctypes.data))
        self._sinks = np.full(n, -1, dtype=np.int32)
        if n:
            _b_int(self._lib.dymu_planner_last_path_sinks(self.h, self._sinks.ctypes.data, n))
        total = max(int(cnt[:n].sum()), 1)
        buf = np.empty((total, 4))
        idx = np.zeros(total, dtype=np.uint32)
        _b_int(fn(self.h, *pre, None, n, 0.0, 0, buf.ctypes.data, idx.ctypes.data, None, None,
                  None))
        ends = np.cumsum(cnt[:n])
        return ([buf[e - c:e].copy() for e, c in zip(ends, cnt[:n])], st[:n].copy(),
                rec[:n].copy(), [idx[e - c:e].copy() for e, c in zip(ends, cnt[:n])])

    def getSimplifiedPaths(self, starts, eps: float, max_wp: int = 1 << 20):
        """getArrivingPaths thinned while the descent runs: every dropped waypoint lies
        within eps (map units) of the segment between the kept waypoints on either side of
        it.  The bound is one-sided (dropped waypoints to the polyline): choose eps below
        the clearance relied on.  max_wp bounds the walk.  Returns (paths, status, records,
        indices): getArrivingPaths' three -- the records are those of the unsimplified
        path -- and per path the uint32 numbers of its waypoints in
        getArrivingPaths(stride=1), whose rows they equal in all four components.
        lastPathSinks / lastPathsOnDevice / lastPathsKernelMs / lastSimplifiedReruns
        report the call."""
        return self._simplified(self._lib.dymu_planner_get_simplified_paths, (), starts, eps,
                                max_wp)

    def getSimplifiedPathsTo(self, b: int, starts, eps: float, max_wp: int = 1 << 20):
        """getSimplifiedPaths on map b of the batch, with goal b as the sink."""
        return self._simplified(self._lib.dymu_planner_get_simplified_paths_to, (b,), starts,
                                eps, max_wp)

    def _last_simplified(self):
        r, b = _u64(), _u64()
        _b_int(self._lib.dymu_planner_last_simplified(self.h, ctypes.byref(r), ctypes.byref(b)))
        return r.value, b.value

    def lastSimplifiedReruns(self) -> int:
        """Paths of the last getSimplifiedPaths[To] that ran a second time on the device
        because they kept more waypoints than the first slot capacity."""
        return self._last_simplified()[0]

    def lastSimplifiedBytes(self) -> int:
        """Bytes of records, counts, slots and indices that call downloaded (0 on the host)."""
        return self._last_simplified()[1]

    # -- every cell's node route to the goal (DyMuPathPlanner::getRouteFields) --
    def _route_fields(self, call, fields, outputs):
        fields = [] if fields is None else list(fields)
        if len(fields) > PATH_FIELDS:
            raise ValueError(f"at most {PATH_FIELDS} fields")
        bad = set(outputs) - set(ROUTE_OUTPUTS)
        if bad:
            raise ValueError(f"unknown outputs {sorted(bad)}; the outputs are {ROUTE_OUTPUTS}")
        keep = []  # the caller's arrays, alive across the call
        fp = (_vp * max(len(fields), 1))()
        for f, a in enumerate(fields):
            if isinstance(a, str):
                if a != "speed":
                    raise ValueError(f"unknown field {a!r}; by name there is 'speed'")
                fp[f] = None
            else:
                keep.append(self._grid(a))
                fp[f] = keep[-1].ctypes.data
        res = {}
        o = DymuRouteOut()
        o.ld = self.nx
        for name, dt in (("sink", np.uint32), ("axis", np.uint32), ("diag", np.uint32),
                         ("length", np.float64)):
            if name in outputs:
                res[name] = np.empty((self.ny, self.nx), dtype=dt)
                setattr(o, name, res[name].ctypes.data)
        for name in ("integral", "vmin", "vmax"):
            if name in outputs:
                res[name] = np.empty((len(fields), self.ny, self.nx))
                arr = getattr(o, name)
                for f in range(len(fields)):
                    arr[f] = res[name][f].ctypes.data
        rounds = _u32()
        _b_int(call(ctypes.cast(fp, _vp), len(fields), o, rounds))
        res["rounds"] = rounds.value
        return res

    def getRouteFields(self, fields=None, outputs=ROUTE_OUTPUTS, host: bool = False) -> dict:
        """Every cell's node route to the goal at once (DyMuPathPlanner::getRouteFields,
        DESIGN.md s5.16): a dict of [ny, nx] maps -- 'sink' (uint32, LABEL_NONE: no route),
        'axis' and 'diag' (hops between axis / diagonal neighbours), 'length' (octile, NaN
        without a route) -- and, stacked [len(fields), ny, nx], 'integral', 'vmin', 'vmax'
        along the route; plus 'rounds'.  fields: up to PATH_FIELDS entries, each 'speed'
        (the speed map the solve used) or a [ny, nx] array.  outputs: the names wanted;
        only they are computed.  The route is the hop-only walk of getArrivingPaths, a chain
        of grid nodes, not its mostly continuous path.  On the GPU while the device map is
        current, else -- or with host=True -- on the host."""
        return self._route_fields(
            lambda fp, n, o, r: self._lib.dymu_planner_get_route_fields(
                self.h, fp, n, int(bool(host)), ctypes.byref(o), ctypes.byref(r)),
            fields, outputs)

    def getRouteFieldsTo(self, b: int, fields=None, outputs=ROUTE_OUTPUTS) -> dict:
        """getRouteFields on map b of the batch, with goal b as the root."""
        return self._route_fields(
            lambda fp, n, o, r: self._lib.dymu_planner_get_route_fields_to(
                self.h, b, fp, n, ctypes.byref(o), ctypes.byref(r)),
            fields, outputs)

    # -- how much of the map drains through every cell (DyMuPathPlanner::getRouteUsage) --
    def _route_usage(self, call, weights, outputs, n_goals):
        bad = set(outputs) - set(USAGE_OUTPUTS)
        if bad:
            raise ValueError(f"unknown outputs {sorted(bad)}; the outputs are {USAGE_OUTPUTS}")
        if not outputs:
            raise ValueError(f"no output asked for; the outputs are {USAGE_OUTPUTS}")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights)
            if w.shape != (self.ny, self.nx):
                raise ValueError(f"weights must be [{self.ny}, {self.nx}], got {w.shape}")
            if w.dtype.kind not in "ui" or (w.size and (w.min() < 0 or w.max() > 0xFFFFFFFF)):
                raise ValueError("weights must be integers in [0, 2^32)")
            w = np.ascontiguousarray(w, dtype=np.uint32)
        res = {}
        o = DymuUsageOut()
        o.ld = self.nx
        for name, dt in (("usage", np.uint64), ("far", np.float64), ("sink", np.uint32)):
            if name in outputs:
                res[name] = np.empty((self.ny, self.nx), dtype=dt)
                setattr(o, name, res[name].ctypes.data)
        cat = None
        if "catchment" in outputs:
            # one spare entry keeps the pointer non-NULL without a goal
            cat = np.zeros(n_goals + 1, dtype=np.uint64)
            res["catchment"] = cat[:n_goals]
        rounds = _u32()
        _b_int(call(w.ctypes.data if w is not None else None, o,
                    cat.ctypes.data if cat is not None else None,
                    len(cat) if cat is not None else 0, rounds))
        res["rounds"] = rounds.value
        return res

    def getRouteUsage(self, weights=None, outputs=USAGE_OUTPUTS, host: bool = False) -> dict:
        """How much of the map drains through every cell (DyMuPathPlanner::getRouteUsage,
        DESIGN.md s5.17): a dict of [ny, nx] maps -- 'usage' (uint64: the weight of all cells
        whose route passes through the cell, itself included), 'far' (the largest total cost
        among them, NaN without a route), 'sink' (uint32, LABEL_NONE: no route) -- plus
        'catchment' (uint64 per goal: the usage at its root, 0 for a dominated goal) and
        'rounds'.  weights: a [ny, nx] array of integers below 2^32, or None for 1 a cell.
        outputs: the names wanted; only they are computed.  On the GPU while the device map
        is current, else -- or with host=True -- on the host; the two are equal bit for bit."""
        n_goals = int(self._lib.dymu_planner_goal_count(self.h))
        return self._route_usage(
            lambda w, o, c, nc, r: self._lib.dymu_planner_get_route_usage(
                self.h, w, int(bool(host)), ctypes.byref(o), c, nc, ctypes.byref(r)),
            weights, outputs, max(n_goals, 0))

    def getRouteUsageTo(self, b: int, weights=None, outputs=USAGE_OUTPUTS) -> dict:
        """getRouteUsage on map b of the batch, with goal b as the root (one catchment)."""
        return self._route_usage(
            lambda w, o, c, nc, r: self._lib.dymu_planner_get_route_usage_to(
                self.h, b, w, ctypes.byref(o), c, nc, ctypes.byref(r)),
            weights, outputs, 1)

    def goalCell(self):
        """(goalI(), goalJ()): the single goal's cell (goal 0 of a goal set), or None."""
        i, j = _u32(), _u32()
        if not _b(self._lib.dymu_planner_goal_cell(self.h, ctypes.byref(i), ctypes.byref(j))):
            return None
        return i.value, j.value

    def goalI(self) -> int:
        return self.goalCell()[0]

    def goalJ(self) -> int:
        return self.goalCell()[1]

    def lastBatchStats(self) -> dict:
        st = DymuStats()
        _check(self._lib.dymu_planner_last_batch_stats(self.h, ctypes.byref(st)))
        return st.as_dict()

    def trackSpeedChanges(self, on: bool = True):
        """Keep the batch and a goal set's map across synchronised speed changes and
        re-propagate them from the changed box; off by default."""
        _check(self._lib.dymu_planner_track_speed_changes(self.h, int(bool(on))))

    def lastBatchSolveKind(self) -> int:
        """0 cold batch solve, 1 windowed re-propagation, 2 batch reused."""
        return _b_int(self._lib.dymu_planner_last_batch_solve_kind(self.h))

    def lastPathsOnDevice(self) -> bool:
        """Whether the last getPaths ran on the device (else on the host threads)."""
        return _b(self._lib.dymu_planner_last_paths_on_device(self.h))

    def lastPathsKernelMs(self) -> float:
        """Kernel time of the last getPaths (HIP events, ms; 0 on the host route)."""
        ms = ctypes.c_double()
        _check(self._lib.dymu_planner_last_paths_kernel_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def getLocomotionMode(self, w) -> str:
        buf = ctypes.create_string_buffer(256)
        _check(min(0, self._lib.dymu_planner_get_locomotion_mode(self.h, *self._wp(w), buf, 256)))
        return buf.value.decode()

    def setGlobalRisk(self, risk_distance: float, risk_ratio: float) -> bool:
        """Obstacle clearance for the global plan: every global solve
        runs on F * (risk_ratio * R + 1), R = max(1 - d / risk_distance, 0) with d the
        distance to the nearest obstacle of the global map.  Either argument 0: off (the
        default).  False: rejected, nothing changed."""
        return _b(self._lib.dymu_planner_set_global_risk(self.h, risk_distance, risk_ratio))

    def getGlobalRiskMatrix(self):
        """R as [j][i]; zeros while the global risk is off."""
        return self._matrix(self._lib.dymu_planner_get_global_risk)

    def setHazardDensity(self, hd) -> bool:
        return _b(self._lib.dymu_planner_set_hazard_density(self.h, self._grid(hd)))

    def setTrafficability(self, tr) -> bool:
        return _b(self._lib.dymu_planner_set_trafficability(self.h, self._grid(tr)))

    def setHazardDensityWindow(self, i0: int, j0: int, hd) -> bool:
        a = np.ascontiguousarray(hd, dtype=np.float64)
        h, w = a.shape
        return _b(self._lib.dymu_planner_set_hazard_density_window(self.h, i0, j0, w, h, a))

    def setTrafficabilityWindow(self, i0: int, j0: int, tr) -> bool:
        a = np.ascontiguousarray(tr, dtype=np.float64)
        h, w = a.shape
        return _b(self._lib.dymu_planner_set_trafficability_window(self.h, i0, j0, w, h, a))

    def setCostMapWindow(self, i0: int, j0: int, cost) -> bool:
        """setCostMap's per-cell rule for the box of `cost` (2-D, [j][i]) at (i0, j0) only:
        the rows of the box alone are re-packed, and with the global risk on obstacles the
        box adds reach R through the incremental update."""
        a = np.ascontiguousarray(cost, dtype=np.float64)
        h, w = a.shape
        return _b(self._lib.dymu_planner_set_cost_map_window(self.h, i0, j0, w, h, a))

    def trackObstacleRemoval(self, on: bool = True) -> None:
        """Off by default.  On: with the global risk on and R current, an obstacle a later
        setCostMapWindow frees reaches R through the incremental update too
        (dymu_clearance_edit_device, lastRiskUpdateKind() == 3) instead of the whole
        clearance solve."""
        _check(self._lib.dymu_planner_track_obstacle_removal(self.h, 1 if on else 0))

    def lastRiskUpdateKind(self) -> int:
        """How R was last brought up to date: 0 not yet, 1 whole solve, 2 incremental after
        obstacles were added, 3 incremental after obstacles were freed (trackObstacleRemoval),
        with or without others added."""
        return _b_int(self._lib.dymu_planner_last_risk_update_kind(self.h))

    def lastRiskUpdate(self) -> dict:
        """The engine's statistics of the last clearance solve or update, with "box": the
        (i0, j0, w, h) of R it rewrote."""
        st = DymuStats()
        box = (_u32 * 4)()
        _check(self._lib.dymu_planner_last_risk_update(self.h, ctypes.byref(st), box))
        d = st.as_dict()
        d["box"] = tuple(int(v) for v in box)
        return d

    def lastRiskRaise(self) -> dict:
        """The raise of the last update of kind 3 (Engine.last_update_stats' figures); zeros
        after any other kind."""
        out = (_u64 * 4)()
        _check(self._lib.dymu_planner_last_risk_raise(self.h, out))
        return {"raise_passes": out[0], "raise_visits": out[1], "cells_invalidated": out[2]}

    def lastBandSize(self) -> int:
        """Narrow-band cells left by the last computeTotalCostMap (0 after a full solve)."""
        return _b_int(self._lib.dymu_planner_last_band_size(self.h))

    def lastSolveKind(self) -> int:
        """0 cold solve, 1 windowed re-propagation, 2 previous map reused."""
        return _b_int(self._lib.dymu_planner_last_solve_kind(self.h))

    def lastEarlyExit(self) -> dict:
        """How the last computeTotalCostMap resolved the reference's pop order at its
        exit value: tied cells, those left OPEN, whether the exact host replay ran
        (degenerate ties only), host milliseconds of the resolution and band replay."""
        o = np.zeros(8)
        _check(self._lib.dymu_planner_last_early_exit_ex(self.h, o.ctypes.data, 8))
        return {"tied": int(o[0]), "open_at_limit": int(o[1]), "exact_replay": bool(o[2]),
                "resolve_ms": float(o[3]), "replay_updates": int(o[4]),
                "band_exact": bool(o[5]), "near_ties": int(o[6]), "replay_threads": int(o[7])}

    def lastStats(self) -> dict:
        st = DymuStats()
        _check(self._lib.dymu_planner_last_stats(self.h, ctypes.byref(st)))
        return st.as_dict()

    # ---- node-level access (src/DyMu.hpp:500-518) ----
    def getGlobalNode(self, i: int, j: int):
        """Snapshot dict of node (i, j), or None (the reference's NULL)."""
        n = DymuGlobalNode()
        if not _b(self._lib.dymu_planner_get_global_node(self.h, i, j, ctypes.byref(n))):
            return None
        return {f: getattr(n, f) for f, _ in DymuGlobalNode._fields_}

    def isSafeNode(self, i: int, j: int) -> bool:
        return _b(self._lib.dymu_planner_is_safe_node(self.h, i, j))

    def isFullyClosedNode(self, i: int, j: int) -> bool:
        return _b(self._lib.dymu_planner_is_fully_closed_node(self.h, i, j))

    def resetTotalCostMap(self):
        _check(self._lib.dymu_planner_reset_total_cost_map(self.h))

    def globalNarrowband(self) -> np.ndarray:
        """global_narrowband (:445) after computeTotalCostMap: (n, 2) array of (i, j)."""
        n = self._lib.dymu_planner_global_narrowband(self.h, None, 0)
        if n < 0:
            _check(int(n))
        ij = np.zeros((max(n, 1), 2), dtype=np.uint32)
        m = self._lib.dymu_planner_global_narrowband(self.h, ij.ctypes.data, n)
        if m < 0:
            _check(int(m))
        return ij[:min(n, m)]

    def minCostGlobalNode(self):
        """minCostGlobalNode (:548-567): ((i, j), total_cost) of the band's lowest
        node, removed from the band list; None on an empty band."""
        ij = np.zeros(2, dtype=np.uint32)
        t = np.zeros(1)
        if not _b(self._lib.dymu_planner_min_cost_global_node(self.h, ij.ctypes.data, t)):
            return None
        return (int(ij[0]), int(ij[1])), float(t[0])

    def resetGlobalNarrowBand(self):
        _check(self._lib.dymu_planner_reset_global_narrow_band(self.h))

    def propagateGlobalNode(self, i: int, j: int):
        """propagateGlobalNode (:500-546) on node (i, j) (host copy of the map)."""
        _check(self._lib.dymu_planner_propagate_global_node(self.h, i, j))

    def setGlobalNodeState(self, i: int, j: int, closed: bool):
        """The public globalNode::state: CLOSED (True) or OPEN."""
        _check(self._lib.dymu_planner_set_global_node_state(self.h, i, j, 1 if closed else 0))

    def nodeStates(self) -> np.ndarray:
        """Every node's state, [ny, nx] uint8 (1 CLOSED, 0 OPEN)."""
        out = np.empty((self.ny, self.nx), dtype=np.uint8)
        _check(self._lib.dymu_planner_get_node_states(self.h, out.ctypes.data))
        return out

    def globalPropagatedNodes(self) -> np.ndarray:
        """global_propagated_nodes (:447): (n, 2) array of (i, j)."""
        n = self._lib.dymu_planner_global_propagated_nodes(self.h, None, 0)
        if n < 0:
            _check(int(n))
        ij = np.zeros((max(n, 1), 2), dtype=np.uint32)
        m = self._lib.dymu_planner_global_propagated_nodes(self.h, ij.ctypes.data, n)
        if m < 0:
            _check(int(m))
        return ij[:min(n, m)]

    # the local layer's per-node steps (L:525-805); nodes are dicts with an "id"
    def _local(self, fn, *args):
        n = DymuLocalNode()
        if not _b(fn(self.h, *args, ctypes.byref(n))):
            return None
        return n.as_dict()

    def getLocalNode(self, x: float, y: float):
        """getLocalNode(Waypoint) (L:177-189; subdivides): dict or None."""
        return self._local(self._lib.dymu_planner_get_local_node, float(x), float(y))

    def localNeighbour(self, node, d: int):
        """node's nb4List[d] (0 (i,j-1), 1 (i-1,j), 2 (i+1,j), 3 (i,j+1)), or None."""
        return self._local(self._lib.dymu_planner_local_neighbour, int(node["id"]), int(d))

    def maxRiskNode(self):
        return self._local(self._lib.dymu_planner_max_risk_node)

    def propagateRisk(self, node):
        _check(self._lib.dymu_planner_propagate_risk(self.h, int(node["id"])))

    def propagateLocalNode(self, node):
        _check(self._lib.dymu_planner_propagate_local_node(self.h, int(node["id"])))

    def setLocalNodeState(self, node, closed: bool):
        _check(self._lib.dymu_planner_set_local_node_state(self.h, int(node["id"]),
                                                           1 if closed else 0))

    def minCostLocalNode(self, Tovertake=None, minC=None, reach=None):
        """minCostLocalNode(Tovertake, minC) (SWEEPING key) or minCostLocalNode(reach)
        (CONSERVATIVE key: deviation + distance to reach)."""
        if reach is not None:
            return self._local(self._lib.dymu_planner_min_cost_local_node_reach, int(reach["id"]))
        return self._local(self._lib.dymu_planner_min_cost_local_node, float(Tovertake or 0.0),
                           float(minC or 0.0))

    def _local_list(self, which: int) -> list:
        n = self._lib.dymu_planner_local_list(self.h, which, None, 0)
        if n < 0:
            _check(int(n))
        arr = (DymuLocalNode * max(n, 1))()
        m = self._lib.dymu_planner_local_list(self.h, which, arr, n)
        if m < 0:
            _check(int(m))
        return [arr[q].as_dict() for q in range(min(n, m))]

    def localNarrowband(self) -> list:
        return self._local_list(0)

    def localExpandableObstacles(self) -> list:
        return self._local_list(1)

    def localPropagatedNodes(self) -> list:
        return self._local_list(2)

    def gradientNode(self, i: int, j: int):
        """gradientNode (:718-772): (dnx, dny)."""
        d = np.zeros(2)
        _check(self._lib.dymu_planner_gradient_node(self.h, i, j, d))
        return float(d[0]), float(d[1])

    def computeLocalWaypointDijkstra(self, w):
        """L:851-869 from the sub-cell at waypoint w: (x, y, z, heading), or None."""
        s = np.array(self._wp(w))
        out = np.zeros(4)
        if not _b(self._lib.dymu_planner_local_waypoint_dijkstra(self.h, s, out)):
            return None
        return tuple(float(v) for v in out)

    def localAgent(self):
        """local_agent's global pose (x, y), or None."""
        xy = np.zeros(2)
        if not _b(self._lib.dymu_planner_local_agent(self.h, xy)):
            return None
        return float(xy[0]), float(xy[1])

    def loadTotalCostMap(self, T) -> bool:
        return _b(self._lib.dymu_planner_load_total_cost_map(self.h, self._grid(T)))

    @property
    def current_path(self) -> np.ndarray:
        n = _b_int(self._lib.dymu_planner_get_current_path(self.h, np.empty(0), 0))
        buf = np.empty(4 * max(n, 1))
        self._lib.dymu_planner_get_current_path(self.h, buf, n)
        return buf[:4 * n].reshape(-1, 4).copy()

    @current_path.setter
    def current_path(self, wps):
        a = np.ascontiguousarray(np.asarray(wps, dtype=np.float64).reshape(-1, 4))
        _check(self._lib.dymu_planner_set_current_path(self.h, a.ctypes.data, len(a)))

    # ---- local layer (src/DyMu_LocalPathRepairing.cpp) ----
    def computeLocalPlanning(self, w, image, res):
        """image: uint8 [height, width] (nonzero = obstacle) or [height, width,
        pixel_size].  Returns (repaired, trajectory [n, 4], local_time_s)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, wd = img.shape[:2]
        ps = img.shape[2] if img.ndim == 3 else 1
        cap = max(64, 4 * len(self.current_path) + 4096)
        buf = np.empty(4 * cap)
        n = ctypes.c_int32()
        t = ctypes.c_double()
        r = _b(self._lib.dymu_planner_compute_local_planning(
            self.h, *self._wp(w), img.ctypes.data, wd, h, wd * ps, ps, res, buf, cap,
            ctypes.byref(n), ctypes.byref(t)))
        if not r:
            return False, np.empty((0, 4)), 0.0
        if n.value > cap:
            return True, self.current_path, t.value
        return True, buf[:4 * n.value].reshape(-1, 4).copy(), t.value

    def repairPath(self, w, index: int) -> int:
        rc = self._lib.dymu_planner_repair_path(self.h, *self._wp(w), index)
        if rc < -1:
            raise DymuError(rc)
        return rc

    def evaluatePath(self, starting_index: int) -> bool:
        return _b(self._lib.dymu_planner_evaluate_path(self.h, starting_index))

    def expandRisk(self):
        _check(self._lib.dymu_planner_expand_risk(self.h))

    def setLocalPropagationTimeout(self, seconds: float):
        """computeLocalPropagation's wall-clock limit (reference: 5 s, <= 0: none)."""
        _check(self._lib.dymu_planner_set_local_timeout(self.h, float(seconds)))

    def computeLocalPropagation(self, w_init, w_overtake):
        """The set node's global pose (x, y), or None."""
        s = np.array(self._wp(w_init))
        o = np.array(self._wp(w_overtake))
        xy = np.empty(2)
        if not _b(self._lib.dymu_planner_compute_local_propagation(self.h, s, o, xy)):
            return None
        return float(xy[0]), float(xy[1])

    def resRatio(self) -> int:
        return _b_int(self._lib.dymu_planner_res_ratio(self.h))

    def _window(self, fn, w):
        ls = 21 * self.resRatio()
        out = np.empty((ls, ls))
        _check(fn(self.h, *self._wp(w), out))
        return out

    def getRiskMatrix(self, w):
        return self._window(self._lib.dymu_planner_get_risk_matrix, w)

    def getDeviationMatrix(self, w):
        return self._window(self._lib.dymu_planner_get_deviation_matrix, w)

    def getReconnectingIndex(self) -> int:
        return self._lib.dymu_planner_get_reconnecting_index(self.h)

    def localMapMask(self):
        m = np.zeros((self.ny, self.nx), dtype=np.uint8)
        _b_int(self._lib.dymu_planner_local_map_mask(self.h, m.ctypes.data))
        return m

    def localBlock(self, i: int, j: int):
        """(dev, tc, risk, state, obst) of node (i, j)'s r x r sub-cells, or None."""
        r = self.resRatio()
        dev, tc, risk = (np.empty((r, r)) for _ in range(3))
        st, ob = (np.empty((r, r), dtype=np.uint8) for _ in range(2))
        if not _b(self._lib.dymu_planner_local_block(self.h, i, j, dev.ctypes.data,
                                                    tc.ctypes.data, risk.ctypes.data,
                                                    st.ctypes.data, ob.ctypes.data)):
            return None
        return dev, tc, risk, st, ob

