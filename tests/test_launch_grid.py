"""grid_rows() of csrc/launch_grid.h, built for the host (tests/cpp/launch_grid_shim.cpp): the two-dimensional grid of every
element-wise kernel covers its lanes, wastes less than one grid row, keeps x * threads inside the 32 bits of a dispatch packet
and y inside 65535, and refuses exactly the counts that would need more rows.  No device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ROWS = 65535


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "launch_grid_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-I/opt/rocm/include",
                           "-D__HIP_PLATFORM_AMD__", "-o", so, os.path.join(ROOT, "tests", "cpp", "launch_grid_shim.cpp")])
    l = C.CDLL(so)
    l.shim_grid_rows.argtypes = [C.c_uint64, C.c_uint, C.POINTER(C.c_uint32)]
    l.shim_grid_rows.restype = C.c_int
    l.shim_grid_row.restype = C.c_uint64
    return l


def grid(shim, lanes, threads):
    out = (C.c_uint32 * 3)()
    return None if shim.shim_grid_rows(lanes, threads, out) else tuple(out)


def test_the_row_is_two_to_the_twenty_workgroups(shim):
    assert shim.shim_grid_row() == 2**20


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_grid_rows_covers_the_lanes_without_a_spare_row(shim, threads):
    row = threads * 2**20                 # lanes of one full grid row
    last = MAX_ROWS * row                 # the most lanes a grid holds
    for lanes in (1, row - 1, row, row + 1, 2**32 - 1, 2**32, 2**32 + 1, 2**28 + 3 * 256 + 77, last - 1, last):
        g = grid(shim, lanes, threads)
        assert g is not None, lanes
        x, y, z = g
        assert z == 1 and x >= 1 and y >= 1
        assert x * y * threads >= lanes, (lanes, g)          # every lane has a thread
        assert (y - 1) * x * threads < lanes, (lanes, g)     # and the last row is needed
        assert x * threads < 2**32, (lanes, g)               # grid_size_x of the dispatch packet
        assert y <= MAX_ROWS, (lanes, g)
        if lanes <= row:
            assert y == 1 and (x - 1) * threads < lanes      # one row: no spare workgroup either
        else:
            assert x == 2**20                                # kernels take blockIdx.y * gridDim.x + blockIdx.x
    # the refusal begins exactly one lane past the last grid, and leaves the grid alone
    assert grid(shim, last + 1, threads) is None
    assert grid(shim, 2**64 - threads, threads) is None


def test_a_second_row_starts_one_lane_past_the_first(shim):
    for threads in (256, 512, 1024):
        row = threads * 2**20
        assert grid(shim, row, threads) == (2**20, 1, 1)
        assert grid(shim, row + 1, threads) == (2**20, 2, 1)
        assert grid(shim, 2 * row, threads) == (2**20, 2, 1)
        assert grid(shim, 2 * row + 1, threads) == (2**20, 3, 1)
    # the count of tests/test_wide_offsets_gpu.py: 2^20 + 4 workgroups of 256
    assert grid(shim, 2**28 + 3 * 256 + 77, 256) == (2**20, 2, 1)
