"""The two planners of the batched pixel calls (csrc/pixel_batch_plan.h, pure host functions) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/pixel_batch_plan_main.cpp, a stand-alone program with its own main, plans the no-device
cases of tests/test_pixels_batch_plan.py.  Built here as the shims of tests/cpp are built, run as its own process; no device."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rocm_include():
    """the directory of hip/hip_runtime_api.h (the planners' headers name hipStream_t and hipError_t; nothing of HIP is called)"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for root in (os.environ.get("ROCM_PATH"), os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    raise AssertionError("no HIP headers: the library itself could not have been built")


def test_the_planners_run_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "pixel_batch_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include(),
                           os.path.join(ROOT, "tests", "cpp", "pixel_batch_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", (r.returncode, r.stdout, r.stderr)
