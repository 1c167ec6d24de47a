"""Records tests/golden/ref_*.npz from the reference planner itself.

Each file holds one case of tests/ref_cases.py: its synthetic inputs and what
oracle/_ref/ref_driver -- the reference's own two sources, compiled unmodified by
`make -C oracle ref` against the stand-in headers in oracle/ref_harness/ -- wrote for
them.  No value in these files comes from oracle/*.c.  Every case runs twice and is
written only if the two runs agree byte for byte (the local layer has wall-clock
bail-outs, and the reference may read memory it never set).  Needs the reference's
sources (REF_SRC of oracle/Makefile).  Run from the repository root:
    python tests/golden/gen_golden_ref.py
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ref_cases  # noqa: E402
import ref_ffi  # noqa: E402

LIMIT = 512 * 1024


def identical(a, b):
    return sorted(a) == sorted(b) and all(
        a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        for k in a)


def check_coverage(name, case, out):
    """the properties a case was drawn for, so that a changed generator cannot quietly
    lose them"""
    if case["family"] == "setcost":
        rc = out["rc_goal_probes"][:, 0]
        assert rc[:10].sum() == 0 and rc[10:].all(), (name, rc)
    if case["family"] == "early":
        assert len(out["narrowband_1"]) > 0 and len(out["narrowband_2"]) > 0, name
        assert (out["total_cost_1"] == -1).any(), name
    if case["family"] == "path":
        p, k, kinds = case["params"], 0, set()
        for n in out["path_len"]:
            w = out["path_wp"][k:k + n]
            k += n
            if n == 0:
                kinds.add("nan at the first step")
            elif n == 2:
                kinds.add("next to the goal")
            else:
                gap = np.hypot(*(w[-1, :2] - w[-2, :2])) / p["gres"]
                kinds.add("nan on the way" if gap > 3 else "stalled" if gap < 0.5 else "complete")
        assert {"nan at the first step", "next to the goal", "nan on the way",
                "complete"} <= kinds, (name, kinds)
        assert np.isinf(out["point_cost"]).any(), name
    if case["family"] == "local":
        assert out["rc_local"][0] == 1 and len(out["trajectory"]) > 20, name


def main():
    if not ref_ffi.have_driver():
        sys.exit("oracle/_ref/ref_driver is missing: run `make -C oracle ref` where the "
                 "reference's sources are")
    for name, case in ref_cases.committed_cases().items():
        second = copy.deepcopy(case)
        a = ref_cases.run_reference(case)
        b = ref_cases.run_reference(second)
        if not identical(a, b):
            sys.exit(f"{name}: two runs of the reference differ; nothing written")
        check_coverage(name, case, a)
        ref_cases.save_fixture(name, case, a)
        size = os.path.getsize(ref_cases.fixture_path(name))
        assert size <= LIMIT, (name, size)
        print(f"{name}: {len(a)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
