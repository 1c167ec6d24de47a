"""AddressSanitizer + UndefinedBehaviorSanitizer build of getSimplifiedPaths' host route
(DyMuPathPlanner::descendArriving with the rule of csrc/path_simplify.h):
the planner sources and the oracle, driven by the stand-alone program
tests/sanitize/simplify_driver.cpp through the flat C-ABI.  The HIP engine is replaced by
tests/sanitize/engine_stub.c, so no GPU runtime enters the sanitized process and every call
takes the host route.  The program is run directly; nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs gcc/g++")
def test_simplified_paths_under_asan_ubsan(tmp_path):
    inc = ["-I" + os.path.join(ROOT, d) for d in ("include", "oracle",
                                                 "planning-path_planning_amd/csrc")]
    objs = []
    for src in ("oracle/oracle.c", "tests/sanitize/engine_stub.c"):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run(["gcc", *FLAGS, "-std=gnu11", *inc, "-c", os.path.join(ROOT, src), "-o", o],
                       check=True)
        objs.append(o)
    exe = str(tmp_path / "simplify_driver")
    srcs = [os.path.join(ROOT, s) for s in (
        "tests/sanitize/simplify_driver.cpp", "planning-path_planning_amd/csrc/planner.cpp",
        "planning-path_planning_amd/csrc/local_layer.cpp",
        "planning-path_planning_amd/csrc/planner_capi.cpp")]
    subprocess.run(["g++", *FLAGS, "-std=c++17", *inc, *srcs, *objs, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "simplify sanitize driver ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
