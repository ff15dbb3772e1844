"""Builds and runs the C++ test program of the BC4 / BC5 image wrappers (tests/cpp/test_cpp_channel_image.cpp) against the
in-tree library, the way tests/test_cpp_api.py builds its program (plus the HIP runtime, for the device-pointer wrappers)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(pkg, tmp_path_factory):
    libdir = os.path.dirname(pkg._lib.lib_path())
    out = str(tmp_path_factory.mktemp("cpp") / "test_cpp_channel_image")
    src = os.path.join(ROOT, "tests", "cpp", "test_cpp_channel_image.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", out, src, f"-L{libdir}", "-ldxtlt_gfx950",
                           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_cpp_channel_image_validation_paths(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_channel_image_on_device(exe):
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
