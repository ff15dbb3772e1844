"""Several images of one BC7 buffer (include/dxtlt_bc7_image.h), everything that needs no GPU: every argument check of the three
calls in the documented order, on made-up addresses that are never dereferenced, with the defective region first, in the middle
and last; the launch plan the debug call reports against a plain Python statement of it; the generic region calls still refusing
format 7; and one compile-and-link use of the three C++ wrappers."""
import os
import subprocess

import pytest

from bc7_image_regions_common import (E_ARGUMENT, E_LENGTH, FACE_BLOCKS, GRANULE, OK, THREE_FACES, TOTAL_THREE, TOTAL_TWO, TWO_FACES,
                                      Launch, groups_of, load, plan_of)
from image_regions_common import CHAIN_256, PER_LAUNCH, TOTAL_256, region_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC, DST = 0x7F1000000000, 0x7F2000000000   # made up


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


def why(lib):
    return lib.dxtlt_last_error().decode()


def calls(lib, src, total, arr, count):
    """(status, reason) of the three calls for one argument set (the host call with len = 16 * total)"""
    out = []
    for call in (lambda: lib.dxtlt_untransform_decode_bc7_images_device(src, total, arr, count, None),
                 lambda: lib.dxtlt_decode_bc7_images_device(src, total, arr, count, None),
                 lambda: lib.dxtlt_untransform_decode_bc7_images(src, 16 * total, arr, count)):
        rc = call()
        out.append((rc, why(lib) if rc != OK else ""))
    return out


def refused(lib, src, total, arr, count, word):
    got = calls(lib, src, total, arr, count)
    assert [rc for rc, _ in got] == [E_ARGUMENT] * 3 and all(word in text for _, text in got), (word, got)


def array_of(regions):
    """regions as (first, width, height, pixels, pitch)"""
    return region_array([r[:3] for r in regions], [r[3] for r in regions], [r[4] for r in regions])


GOOD = [(0, 8, 8, DST, 32), (10, 8, 8, DST + 4096, 36), (20, 8, 8, DST + 8192, 48)]   # 4 blocks each, of 100
# a defect of every kind for the region at `first`, in the documented order, and a word of its reason
DEFECTS = [
    ("NULL pixels", lambda first: (first, 8, 8, None, 32)),
    ("smaller", lambda first: (first, 8, 8, DST + 0x100000, 28)),
    ("smaller", lambda first: (first, 0x40000001, 1, DST + 0x100000, 16)),        # 4 * width needs 33 bits
    ("multiples", lambda first: (first, 8, 8, DST + 0x100000, 34)),
    ("multiples", lambda first: (first, 8, 8, DST + 0x100002, 32)),
    ("total_blocks", lambda first: (first, 8, 400, DST + 0x100000, 32)),          # 200 blocks of 100
    ("total_blocks", lambda first: (2**64 - 2, 8, 8, DST + 0x100000, 32)),        # first_block + blocks wraps
]


@pytest.mark.parametrize("at", [0, 1, 2])
def test_every_region_defect_first_in_the_middle_and_last(lib, at):
    for word, make in DEFECTS:
        regions = list(GOOD)
        regions[at] = make(GOOD[at][0])
        refused(lib, SRC, 100, array_of(regions), 3, word)
    # a region that starts before the previous non-empty one ends: overlapping, descending, the same range twice -- the first
    # region has none in front of it
    if at > 0:
        before = GOOD[at - 1][0]
        for first in [before + 3, before] + ([before - 5] if before >= 5 else []):
            regions = list(GOOD)
            regions[at] = (first,) + GOOD[at][1:]
            refused(lib, SRC, 100, array_of(regions), 3, "ascending")
    # an empty region between two others is skipped, whatever it holds: the overlap of the two around it is still found
    regions = [GOOD[0], (2**64 - 1, 0, 0, None, 0), (2,) + GOOD[1][1:]]
    refused(lib, SRC, 100, array_of(regions), 3, "ascending")


def test_the_checks_come_in_the_documented_order(lib):
    one = lambda *r: array_of([r])
    # 1. no regions, or only empty ones: OK whatever else is passed -- NULL pointers, a length that is no multiple of 16
    assert [rc for rc, _ in calls(lib, None, 0, None, 0)] == [OK] * 3
    assert [rc for rc, _ in calls(lib, None, 0, array_of(GOOD), 0)] == [OK] * 3
    empty = array_of([(2**64 - 1, 0, 8, None, 0), (5, 8, 0, 1, 1), (2**63, 0, 0, DST, 3)])
    assert [rc for rc, _ in calls(lib, None, 0, empty, 3)] == [OK] * 3
    assert lib.dxtlt_untransform_decode_bc7_images(None, 3, empty, 3) == OK
    assert lib.dxtlt_untransform_decode_bc7_images(None, 3, None, 0) == OK
    # 2. a NULL buffer or regions pointer, before anything about a region
    bad_everywhere = one(2**64 - 2, 8, 8, None, 1)           # NULL pixels, a small pitch, a range that wraps
    refused(lib, None, 4, bad_everywhere, 1, "NULL buffer")
    refused(lib, SRC, 4, None, 1, "NULL regions")
    refused(lib, None, 4, one(0, 8, 8, DST, 32), 1, "NULL buffer")
    # 3. inside a region: NULL pixels, then the pitch, then the multiples, then the range, then the order
    refused(lib, SRC, 4, bad_everywhere, 1, "NULL pixels")
    refused(lib, SRC, 4, one(2**64 - 2, 8, 8, DST + 1, 30), 1, "smaller")
    refused(lib, SRC, 4, one(2**64 - 2, 8, 8, DST + 1, 33), 1, "multiples")
    refused(lib, SRC, 3, one(0, 8, 8, DST, 32), 1, "total_blocks")
    refused(lib, SRC, 100, array_of([GOOD[1], (9, 8, 400, DST, 32)]), 2, "total_blocks")    # out of range AND out of order
    refused(lib, SRC, 100, array_of([GOOD[1], (9, 8, 8, DST, 32)]), 2, "ascending")
    # across regions the list order decides: the earlier region's late kind of defect is the answer, not the later region's early kind
    refused(lib, SRC, 100, array_of([(98, 8, 8, DST, 32), (99, 8, 8, None, 1)]), 2, "total_blocks")
    refused(lib, SRC, 100, array_of([GOOD[0], (2, 8, 8, DST + 4096, 32), (50, 8, 8, None, 32)]), 3, "ascending")
    refused(lib, SRC, 100, array_of([GOOD[0], (50, 8, 8, DST + 4096, 30), (2, 8, 8, DST + 8192, 32)]), 3, "smaller")
    # the block pointer may have any alignment: an odd one gets as far as the range
    refused(lib, SRC + 1, 3, one(0, 8, 8, DST + 4, 36), 1, "total_blocks")
    # 4. the host call's length, last
    host = lib.dxtlt_untransform_decode_bc7_images
    good = one(0, 8, 8, DST, 32)
    assert host(SRC, 64 + 3, good, 1) == E_LENGTH
    assert host(SRC, 48 + 3, good, 1) == E_ARGUMENT and "total_blocks" in why(lib)         # the range before the length
    assert host(SRC, 64 + 3, one(0, 8, 8, DST, 31), 1) == E_ARGUMENT
    assert host(SRC, 64 + 3, one(0, 8, 8, None, 32), 1) == E_ARGUMENT
    assert host(SRC, 64 + 3, array_of([(0, 8, 8, DST, 32), (0, 8, 8, DST + 4096, 32)]), 2) == E_ARGUMENT
    assert host(None, 64 + 3, empty, 3) == OK


def test_the_generic_region_calls_still_refuse_bc7(lib):
    good = array_of([(0, 8, 8, DST, 32)])
    for fmt in (6, 7):
        assert lib.dxtlt_untransform_decode_images_device(fmt, SRC, 4, good, 1, 0, False, False, None) == E_ARGUMENT
        assert "format" in why(lib)
        assert lib.dxtlt_decode_images_device(fmt, SRC, 4, good, 1, None) == E_ARGUMENT and "format" in why(lib)
        assert lib.dxtlt_untransform_decode_images(fmt, SRC, 64, good, 1, 0, False, False) == E_ARGUMENT and "format" in why(lib)
        assert lib.dxtlt_decode_images_device(fmt, None, 0, None, 0, None) == E_ARGUMENT           # the format comes first there


# ---- the plan --------------------------------------------------------------------------------------------------------------
def planned(lib, total, regions, cap=64):
    arr = region_array(regions, [DST + 0x1000000 * i for i in range(len(regions))], [4 * r[1] for r in regions])
    out = (Launch * cap)()
    n = lib.dxtlt_debug_plan_bc7_images(total, arr, len(regions), out, cap)
    assert 0 <= n <= cap and all(out[i].reserved == 0 for i in range(n))
    return [(o.first_region, o.region_count, o.first_granule, o.granule_count, o.tail) for o in out[:n]]


def test_plan_of_the_chain_and_the_faces(lib):
    # the 256 x 256 nine-level chain: one main launch of 5 granules and one tail launch
    assert planned(lib, TOTAL_256, CHAIN_256) == [(0, 9, 0, 5, 0), (0, 9, 5, 1, 1)] == plan_of(TOTAL_256, CHAIN_256)
    # two faces: sixteen regions, one group, both main granules and the tail part
    assert planned(lib, TOTAL_TWO, TWO_FACES) == [(0, 16, 0, 2, 0), (0, 16, 2, 1, 1)] == plan_of(TOTAL_TWO, TWO_FACES)
    # three faces: two groups, granule 2 in both
    assert [len(g) for _, g in groups_of(THREE_FACES)] == [PER_LAUNCH, 8] and 2 * FACE_BLOCKS // GRANULE == 2
    assert planned(lib, TOTAL_THREE, THREE_FACES) == [(0, 16, 0, 3, 0), (16, 8, 2, 2, 0), (16, 8, 4, 1, 1)]
    assert planned(lib, TOTAL_THREE, THREE_FACES) == plan_of(TOTAL_THREE, THREE_FACES)


def test_plan_at_the_edges_of_the_parts(lib):
    # a single region wholly inside the tail part: the tail launch only
    assert planned(lib, TOTAL_256, [CHAIN_256[4]]) == [(0, 1, 5, 1, 1)] == plan_of(TOTAL_256, [CHAIN_256[4]])
    # a range that ends exactly at main_blocks: no tail launch
    assert planned(lib, TOTAL_256, CHAIN_256[:2]) == [(0, 2, 0, 5, 0)] == plan_of(TOTAL_256, CHAIN_256[:2])
    assert planned(lib, 2391, [(2044, 16, 4)]) == [(0, 1, 1, 1, 0)]
    assert planned(lib, 2391, [(2044, 20, 4)]) == [(0, 1, 1, 1, 0), (0, 1, 2, 1, 1)]
    # a group is not split at a gap: blocks 0 and 4000 of the chain's buffer are one launch over granules 0 .. 3
    assert planned(lib, TOTAL_256, [(0, 4, 4), (4000, 4, 4)]) == [(0, 2, 0, 4, 0)]
    for total in (1, 1023, 1024, 1025):
        for regions in ([(0, 4, 4 * total)], [(total - 1, 1, 1)], [(0, 2, 3), (total - 1, 4, 4)] if total > 1 else [(0, 2, 3)]):
            got = planned(lib, total, regions)
            assert got == plan_of(total, regions), (total, regions)
            assert len(got) == (2 if total == 1025 and regions[0][0] == 0 else 1)
            assert got[-1][4] == (1 if total != 1024 else 0)
    # empty regions are no part of a group, wherever their first_block points; the group's index is that of its first real region
    regions = [(2**63, 0, 7), CHAIN_256[0], (2**63, 5, 0), CHAIN_256[2], (5400, 0, 0), CHAIN_256[5]]
    assert planned(lib, TOTAL_256, regions) == [(1, 3, 0, 5, 0), (1, 3, 5, 1, 1)] == plan_of(TOTAL_256, regions)
    assert planned(lib, TOTAL_256, [(2**63, 0, 7)]) == [] and planned(lib, TOTAL_256, []) == []


def test_plan_counts_beyond_the_capacity_and_refuses_what_the_call_refuses(lib):
    arr = region_array(THREE_FACES, [DST + 0x1000000 * i for i in range(24)], [4 * r[1] for r in THREE_FACES])
    assert lib.dxtlt_debug_plan_bc7_images(TOTAL_THREE, arr, 24, None, 0) == 3
    out = (Launch * 2)()
    assert lib.dxtlt_debug_plan_bc7_images(TOTAL_THREE, arr, 24, out, 2) == 3 and (out[1].first_region, out[1].first_granule) == (16, 2)
    assert lib.dxtlt_debug_plan_bc7_images(TOTAL_THREE - 1, arr, 24, out, 2) == -1           # the last region does not fit
    assert lib.dxtlt_debug_plan_bc7_images(TOTAL_THREE, None, 24, out, 2) == -1
    bad = array_of([GOOD[1], GOOD[0]])
    assert lib.dxtlt_debug_plan_bc7_images(100, bad, 2, out, 2) == -1 and "ascending" in why(lib)
    assert lib.dxtlt_debug_plan_bc7_images(100, array_of([(0, 8, 8, None, 32)]), 1, out, 2) == -1


# ---- Python and C++ ---------------------------------------------------------------------------------------------------------
def test_python_module_exposes_the_bc7_region_calls(pkg):
    import numpy as np

    from dxt_lossless_transform_amd import image

    with pytest.raises(TypeError):
        image.decode_bc7_images(np.zeros(16, np.uint8), [(0, 4, 4)])   # device tensors only
    with pytest.raises(pkg.InvalidLength):
        image.untransform_decode_bc7_images(np.zeros(17, np.uint8), [(0, 4, 4)])
    with pytest.raises(pkg.DeviceError):
        image.untransform_decode_bc7_images(np.zeros(16, np.uint8), [(1, 4, 4)])   # the region is not in the buffer
    # a list without a non-empty region needs no device
    outs = image.untransform_decode_bc7_images(np.zeros(16, np.uint8), [(0, 0, 4), (7, 4, 0)])
    assert [o.size for o in outs] == [0, 0]
    assert image.untransform_decode_bc7_images(np.zeros(16, np.uint8), []) == []


def test_cpp_wrappers_compile_link_and_check_their_arguments(pkg, tmp_path):
    libdir = os.path.dirname(pkg._lib.lib_path())
    exe = str(tmp_path / "test_cpp_bc7_images")
    src = os.path.join(ROOT, "tests", "cpp", "test_cpp_bc7_images.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, src, f"-L{libdir}", "-ldxtlt_gfx950",
                           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
