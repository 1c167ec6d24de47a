#!/usr/bin/env python3
"""Probe of the wrong map after an engine has grown.

One kernel-5 engine (prio_target = 16) per sequence: a first grid of ones, then the MT19937
grids at 256^2, 512^2 and 1024^2 with the goal in the centre, each map checked against the
KAT sums of tests/test_gpu_solver.py.  Forms (any number, run in the order given, `tries`
engines each, all in one process -- the order matters, see DESIGN):

  host       dymu_solve on host arrays (the staged maps grow with every grid)
  host_then  host, then at 1024^2: host again, a device-form solve, host a third time
  keep       dymu_solve_device on two caller buffers allocated once for 1024^2
  realloc    the same with the buffers freed and allocated at the grid's size per grid
The device forms read the speed back after the solve and compare it with the upload.

--det: deterministic=1 engines, device forms only, stepped.  A fresh engine solves 1024^2
last and records, every --every passes, hashes of the map, the next list, the keys, the
stamps (relative to eb) and the edge columns, and the per-pass statistics; every sequence's
1024^2 solve is compared with it and the first differing pass is printed per field.

  python tools/history_probe.py [--first 48] [--tries 2] [--det] [--every 16] FORM...
One JSON line per solve on stdout.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "planning-path_planning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dymu  # noqa: E402
import oracle_ffi  # noqa: E402

KAT = {256: "1.7066083890e+07", 512: "1.3467278246e+08", 1024: "1.0666255888e+09"}
OPTS = dict(kernel=5, prio_target=16)


def kat(T):
    N = T.shape[0]
    s = f"{np.where(np.isinf(T), -1.0, T).sum():.10e}"
    return True if N not in KAT or s == KAT[N] else s


def h(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


class Bufs:
    def __init__(self, eng, realloc):
        self.eng, self.realloc, self.p = eng, realloc, []

    def get(self, F):
        if self.realloc or not self.p:
            self.free()
            self.p = [self.eng.alloc(F.nbytes if self.realloc else 8 << 20) for _ in range(2)]
        return self.p

    def free(self):
        for q in self.p:
            self.eng.free(q)
        self.p = []


def dev_solve(eng, bufs, F, trace=None, every=16):
    """solve_device on caller buffers; with trace (a list): stepped, a record every `every`
    passes.  Returns T, stats, speed read back intact."""
    N = F.shape[0]
    dF, dT = bufs.get(F)
    eng.h2d(dF, F)
    T = np.empty((N, N))
    if trace is None:
        st = eng.solve_device(dF, dT, N, N, N, N // 2, N // 2)
    else:
        eng.set_stepping(True)
        eng.solve_device(dF, dT, N, N, N, N // 2, N // 2)
        p = 0
        while True:
            pending = eng.dom_pending()
            s = eng.dom_snapshot()
            eng.d2h(T, dT)
            trace.append(dict(p=p, pending=pending, T=h(T), list=h(np.sort(s["list_tile"])),
                              keys=h(s["keys"]), ec=h(s["ec"]),
                              stamps=h(np.maximum(s["tile_epoch"].astype(np.int64) - s["eb"], 0)),
                              hist=h(s["hist"])))
            if pending == 0:
                break
            eng.dom_run(every)
            p += every
        st = eng.dom_finish()
        eng.set_stepping(False)
    eng.d2h(T, dT)
    Fd = np.empty_like(F)
    eng.d2h(Fd, dF)
    return T, st, bool(np.array_equal(Fd.view(np.uint64), F.view(np.uint64)))


def first_diff(ref, got):
    out = {}
    for key in ("pending", "T", "list", "keys", "ec", "stamps", "hist"):
        for a, b in zip(ref, got):
            if a[key] != b[key]:
                out[key] = a["p"]
                break
    if len(ref) != len(got):
        out["records"] = [len(ref), len(got)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("forms", nargs="+", choices=["host", "host_then", "keep", "realloc"])
    ap.add_argument("--first", type=int, default=48)
    ap.add_argument("--tries", type=int, default=2)
    ap.add_argument("--det", action="store_true")
    ap.add_argument("--every", type=int, default=16)
    a = ap.parse_args()
    o = oracle_ffi.load()
    mt = {N: o.mt_uniform(N * N).reshape(N, N) for N in KAT}
    seq = [np.ones((a.first, a.first))] + [mt[N] for N in (256, 512, 1024)]
    opts = dict(OPTS, deterministic=1) if a.det else OPTS

    def say(**kw):
        print(json.dumps(kw), flush=True)

    late = []  # --det: compared with the fresh engine, which runs last
    for form in a.forms:
        if a.det and form.startswith("host"):
            continue
        for k in range(a.tries):
            with dymu.Engine(**opts) as eng:
                bufs = Bufs(eng, form == "realloc")
                if a.det:
                    eng.set_pass_stats(True)
                for F in seq:
                    N = F.shape[0]
                    rec = dict(form=form, attempt=k, N=N)
                    if form.startswith("host"):
                        r = eng.solve(F, N // 2, N // 2)
                        T, st = r.T, r.stats
                    else:
                        trace = [] if a.det and N == 1024 else None
                        T, st, rec["speed_intact"] = dev_solve(eng, bufs, F, trace, a.every)
                        if trace is not None:
                            late.append((form, k, trace, eng.last_pass_stats()))
                    say(passes=st["passes"], visits=st["tile_visits"], kat=kat(T), **rec)
                if form == "host_then":
                    F = mt[1024]
                    r = eng.solve(F, 512, 512)
                    say(form=form, attempt=k, step="host again", passes=r.stats["passes"],
                        kat=kat(r.T))
                    T, st, fok = dev_solve(eng, bufs, F)
                    say(form=form, attempt=k, step="device form after", passes=st["passes"],
                        kat=kat(T), speed_intact=fok)
                    r = eng.solve(F, 512, 512)
                    say(form=form, attempt=k, step="host third", passes=r.stats["passes"],
                        kat=kat(r.T))
                bufs.free()
    if a.det:
        with dymu.Engine(**opts) as eng:
            eng.set_pass_stats(True)
            bufs, ref = Bufs(eng, False), []
            T, st, fok = dev_solve(eng, bufs, mt[1024], ref, a.every)
            ref_ps = eng.last_pass_stats()
            bufs.free()
            say(form="fresh", N=1024, passes=st["passes"], kat=kat(T), speed_intact=fok)
        for form, k, trace, ps in late:
            n = min(len(ps), len(ref_ps))
            d = np.flatnonzero((ps[:n] != ref_ps[:n]).any(axis=1))
            say(form=form, attempt=k, N=1024, first_differing_pass=first_diff(ref, trace),
                first_differing_pass_stats=int(d[0]) if d.size else None,
                pass_stats_there=[ps[d[0]].tolist(), ref_ps[d[0]].tolist()] if d.size else None)


if __name__ == "__main__":
    main()
