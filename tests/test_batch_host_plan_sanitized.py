"""The planner of dxtlt_transform_batch_host (csrc/batch_host_plan.h), a pure host function, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/batch_host_plan_main.cpp, a stand-alone program with its own main, plans the edge lists of
tests/test_batch_host_plan.py, no item at all and lengths near 2^40.  Built and run as tests/test_batch_auto_plan_sanitized.py
builds and runs its program: its own process, no device."""
import os
import subprocess

from test_pixels_batch_plan_sanitized import ROOT


def test_the_host_batch_planner_runs_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "batch_host_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined",   # (no HIP include path: the planner's header names nothing of HIP)
                           os.path.join(ROOT, "tests", "cpp", "batch_host_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", (r.returncode, r.stdout, r.stderr)
