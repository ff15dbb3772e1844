"""The planner of the batched BC1 - BC5 auto call (csrc/batch_auto_plan.h) and what it shares with the batched pixel auto call
(csrc/batch_auto_common.h: the overlap rule, the chunk packer, the estimator's section table), pure host functions, under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/batch_auto_plan_main.cpp, a stand-alone program with its own main, plans
the no-device cases of tests/test_batch_auto_plan.py and checks the tables written for a made-up arena.  Built and run as
tests/test_pixels_batch_plan_sanitized.py builds and runs its program: its own process, no device."""
import os
import subprocess

from test_pixels_batch_plan_sanitized import ROOT, rocm_include


def test_the_block_planner_and_the_shared_pieces_run_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "batch_auto_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include(),
                           os.path.join(ROOT, "tests", "cpp", "batch_auto_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", (r.returncode, r.stdout, r.stderr)
