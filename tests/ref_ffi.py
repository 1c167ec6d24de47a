"""Runs oracle/_ref/ref_driver (TEST INFRASTRUCTURE ONLY): the reference planner's own
sources, compiled by `make -C oracle ref` against the stand-in headers of
oracle/ref_harness/.  The driver exists only where the reference's sources do; the
committed tests/golden/ref_*.npz fixtures are what it recorded.

run(family, params, arrays) -> dict of numpy arrays.  `params` become the `key v0 v1 ...`
lines of the driver's case.txt, `arrays` its in_NAME.bin files.  Keys per family
(all take nx, ny, gres, lres, offset, risk_distance, reconnect_distance, risk_ratio and
optionally approach: 0 conservative, 1 sweeping):

  setcost  cost[ny,nx]; goal (x, y, heading); goal_probes[n,2]
  costmap  lut, slopes, elevation[ny,nx], terrain[ny,nx]; n_locs  (computeCostMap twice)
  early    cost[ny,nx]; goal, start, goal2, start2 (x, y)
  path     costmap's inputs; goal; starts[n,3] (x, y, heading); points[m,2]
  local    costmap's inputs; goal; start; optionally rover (x, y), image[h,w(,ps)],
           image_res
"""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODIR = os.path.join(ROOT, "oracle")
DRIVER = os.path.join(ODIR, "_ref", "ref_driver")
_DT = {"f64": np.float64, "i64": np.int64, "u8": np.uint8}


def ref_src():
    """The directory the oracle Makefile would compile the reference from."""
    r = subprocess.run(["make", "-s", "print-ref-src"], cwd=ODIR, check=True,
                       capture_output=True, text=True)
    return r.stdout.strip()


def have_sources():
    return os.path.exists(os.path.join(ref_src(), "DyMu.hpp"))


def have_driver():
    return os.path.exists(DRIVER)


def _num(v):
    v = float(v)
    return v.hex() if np.isfinite(v) else repr(v)


def run(family, params, arrays):
    with tempfile.TemporaryDirectory(prefix="ref_case_") as d:
        with open(os.path.join(d, "case.txt"), "w") as f:
            f.write(f"family {family}\n")
            for k, v in params.items():
                f.write(k + " " + " ".join(_num(x) for x in np.atleast_1d(v)) + "\n")
        for k, a in arrays.items():
            a = np.asarray(a)
            dt = np.uint8 if a.dtype == np.uint8 else np.float64
            np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, f"in_{k}.bin"))
        r = subprocess.run([DRIVER, d], capture_output=True, text=True, timeout=20)
        if r.returncode != 0:
            raise RuntimeError(f"ref_driver {family}: exit {r.returncode}\n{r.stderr[-2000:]}")
        out = {}
        with open(os.path.join(d, "manifest.txt")) as f:
            for line in f:
                name, dt, *dims = line.split()
                a = np.fromfile(os.path.join(d, f"out_{name}.bin"), dtype=_DT[dt])
                out[name] = a.reshape([int(x) for x in dims]).copy()
        return out
