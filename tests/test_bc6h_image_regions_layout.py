"""Several images of one BC6H buffer (include/dxtlt_bc6h_image.h), everything that needs no GPU: every argument check of the three
calls in the documented order, on made-up addresses that are never dereferenced, with the defective region first, in the middle
and last, alone and in pairs, the return code and the whole dxtlt_last_error() text pinned for the 8-byte pixel; the launch plan
the debug call reports against the plain Python statement of it, and the BC7 debug call's answers beside it; the generic and the
BC7 region calls still refusing format 6; and one compile-and-link use of the three C++ wrappers."""
import os
import subprocess

import pytest

from bc6h_image_regions_common import (CHAIN_256, E_ARGUMENT, E_LENGTH, FACE_BLOCKS, GRANULE, MAX_GRANULES, OK, PER_LAUNCH, THREE_FACES,
                                       TOTAL_256, TOTAL_THREE, TOTAL_TWO, TWO_FACES, Bc7Launch, Launch, groups_of, load, plan_of,
                                       region_array)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC, DST = 0x7F1000000000, 0x7F2000000000   # made up

# the whole texts of the region list's defects (csrc/image_host.h, image_regions_defect), in the documented order
NULL_REGIONS = "dxtlt: NULL regions pointer"
NULL_BUFFER = "dxtlt: NULL buffer with a non-empty region"
NULL_PIXELS = "dxtlt: NULL pixels pointer of a non-empty region"
SMALL_PITCH = "dxtlt: a region's pitch is smaller than the bytes of a pixel row"
MULTIPLES = "dxtlt: a region's pitch and pixel pointer must be multiples of 4 (BC1 - BC3) or of the bytes per pixel"
RANGE = "dxtlt: first_block + blocks of a region exceeds total_blocks"
ORDER = "dxtlt: regions must come in ascending block order and must not overlap"


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


def why(lib):
    return lib.dxtlt_last_error().decode()


def calls(lib, src, total, arr, count):
    """(status, reason) of the three call forms for one argument set (the host call with len = 16 * total)"""
    out = []
    for call in (lambda: lib.dxtlt_untransform_decode_bc6h_images_device(src, total, arr, count, None),
                 lambda: lib.dxtlt_decode_bc6h_images_device(src, total, arr, count, None),
                 lambda: lib.dxtlt_untransform_decode_bc6h_images(src, 16 * total, arr, count)):
        rc = call()
        out.append((rc, why(lib) if rc != OK else ""))
    return out


def refused(lib, src, total, arr, count, text):
    got = calls(lib, src, total, arr, count)
    assert got == [(E_ARGUMENT, text)] * 3, (text, got)


def array_of(regions):
    """regions as (first, width, height, pixels, pitch)"""
    return region_array([r[:3] for r in regions], [r[3] for r in regions], [r[4] for r in regions])


# 4 blocks each, of 100; rows of 64 bytes; pitches that are multiples of 16 and of 8 only
GOOD = [(0, 8, 8, DST, 64), (10, 8, 8, DST + 4096, 72), (20, 8, 8, DST + 8192 + 8, 80)]
# a defect of every kind for the region at `first`, in the documented order, with its text.  The 8-byte rule: a pitch of 60 is
# too small for 8 pixels where 32 would do for four-byte pixels, and 4 is no multiple that will do
DEFECTS = [
    (NULL_PIXELS, lambda first: (first, 8, 8, None, 64)),
    (SMALL_PITCH, lambda first: (first, 8, 8, DST + 0x100000, 60)),
    (SMALL_PITCH, lambda first: (first, 8, 8, DST + 0x100000, 32)),               # 4 * width: an RGBA8888 row
    (SMALL_PITCH, lambda first: (first, 0x20000001, 1, DST + 0x100000, 16)),      # 8 * width needs 33 bits
    (MULTIPLES, lambda first: (first, 8, 8, DST + 0x100000, 68)),                 # pitch a multiple of 4 only
    (MULTIPLES, lambda first: (first, 8, 8, DST + 0x100004, 64)),                 # pointer a multiple of 4 only
    (MULTIPLES, lambda first: (first, 8, 8, DST + 0x100000, 65)),
    (RANGE, lambda first: (first, 8, 400, DST + 0x100000, 64)),                   # 200 blocks of 100
    (RANGE, lambda first: (2**64 - 2, 8, 8, DST + 0x100000, 64)),                 # first_block + blocks wraps
]


@pytest.mark.parametrize("at", [0, 1, 2])
def test_every_region_defect_first_in_the_middle_and_last(lib, at):
    for text, make in DEFECTS:
        regions = list(GOOD)
        regions[at] = make(GOOD[at][0])
        refused(lib, SRC, 100, array_of(regions), 3, text)
    # a region that starts before the previous non-empty one ends: overlapping, descending, the same range twice -- the first
    # region has none in front of it
    if at > 0:
        before = GOOD[at - 1][0]
        for first in [before + 3, before] + ([before - 5] if before >= 5 else []):
            regions = list(GOOD)
            regions[at] = (first,) + GOOD[at][1:]
            refused(lib, SRC, 100, array_of(regions), 3, ORDER)
    # an empty region between two others is skipped, whatever it holds: the overlap of the two around it is still found
    regions = [GOOD[0], (2**64 - 1, 0, 0, None, 0), (2,) + GOOD[1][1:]]
    refused(lib, SRC, 100, array_of(regions), 3, ORDER)
    # the good list is good: pointers and pitches that are multiples of 8 pass the checks in the plan call, which has no device
    assert lib.dxtlt_debug_plan_bc6h_images(100, array_of(GOOD), 3, None, 0) == 1


def test_of_two_defects_the_earlier_check_wins(lib):
    """pairs of defects in ONE region: the answer is the one whose check comes first in the documented order"""
    one = lambda *r: array_of([r])
    kinds = {   # what makes the defect, as overrides of a good (first, width, height, pixels, pitch) for a buffer of 4 blocks
        NULL_PIXELS: {3: None},
        SMALL_PITCH: {4: 56},
        MULTIPLES: {3: DST + 4},
        RANGE: {0: 1},
    }
    order = [NULL_PIXELS, SMALL_PITCH, MULTIPLES, RANGE]
    for i, first in enumerate(order):
        for second in order[i + 1:]:
            region = [0, 8, 8, DST, 64]
            for k, v in {**kinds[second], **kinds[first]}.items():
                region[k] = v
            if first == SMALL_PITCH and second == MULTIPLES:
                region[4] = 60                                  # too small AND no multiple of 8, beside the odd pointer
            refused(lib, SRC, 4, one(*region), 1, first)
    # the order check is the last inside a region: with any other defect in the same region, the other one is the answer
    for text in order:
        region = [2, 8, 8, DST + 4096, 64]                       # starts inside GOOD[0]
        if text == RANGE:
            region[2] = 400                                      # 200 blocks from block 2 of 100
        else:
            for k, v in kinds[text].items():
                region[k] = v
        refused(lib, SRC, 100, array_of([GOOD[0], tuple(region)]), 2, text)


def test_the_checks_come_in_the_documented_order(lib):
    one = lambda *r: array_of([r])
    # 1. no regions, or only empty ones: OK whatever else is passed -- NULL pointers, a length that is no multiple of 16
    assert [rc for rc, _ in calls(lib, None, 0, None, 0)] == [OK] * 3
    assert [rc for rc, _ in calls(lib, None, 0, array_of(GOOD), 0)] == [OK] * 3
    empty = array_of([(2**64 - 1, 0, 8, None, 0), (5, 8, 0, 1, 1), (2**63, 0, 0, DST, 3)])
    assert [rc for rc, _ in calls(lib, None, 0, empty, 3)] == [OK] * 3
    assert lib.dxtlt_untransform_decode_bc6h_images(None, 3, empty, 3) == OK
    assert lib.dxtlt_untransform_decode_bc6h_images(None, 3, None, 0) == OK
    # 2. a NULL buffer or regions pointer, before anything about a region
    bad_everywhere = one(2**64 - 2, 8, 8, None, 1)           # NULL pixels, a small pitch, a range that wraps
    refused(lib, None, 4, bad_everywhere, 1, NULL_BUFFER)
    refused(lib, SRC, 4, None, 1, NULL_REGIONS)
    refused(lib, None, 4, None, 1, NULL_REGIONS)
    refused(lib, None, 4, one(0, 8, 8, DST, 64), 1, NULL_BUFFER)
    # 3. inside a region: NULL pixels, then the pitch, then the multiples, then the range, then the order
    refused(lib, SRC, 4, bad_everywhere, 1, NULL_PIXELS)
    refused(lib, SRC, 4, one(2**64 - 2, 8, 8, DST + 1, 62), 1, SMALL_PITCH)
    refused(lib, SRC, 4, one(2**64 - 2, 8, 8, DST + 1, 65), 1, MULTIPLES)
    refused(lib, SRC, 4, one(2**64 - 2, 8, 8, DST + 4, 64), 1, MULTIPLES)
    refused(lib, SRC, 3, one(0, 8, 8, DST, 64), 1, RANGE)
    refused(lib, SRC, 100, array_of([GOOD[1], (9, 8, 400, DST, 64)]), 2, RANGE)    # out of range AND out of order
    refused(lib, SRC, 100, array_of([GOOD[1], (9, 8, 8, DST, 64)]), 2, ORDER)
    # across regions the list order decides: the earlier region's late kind of defect is the answer, not the later region's early kind
    refused(lib, SRC, 100, array_of([(98, 8, 8, DST, 64), (99, 8, 8, None, 1)]), 2, RANGE)
    refused(lib, SRC, 100, array_of([GOOD[0], (2, 8, 8, DST + 4096, 64), (50, 8, 8, None, 64)]), 3, ORDER)
    refused(lib, SRC, 100, array_of([GOOD[0], (50, 8, 8, DST + 4096, 60), (2, 8, 8, DST + 8192, 64)]), 3, SMALL_PITCH)
    # the block pointer may have any alignment: an odd one gets as far as the range
    refused(lib, SRC + 1, 3, one(0, 8, 8, DST + 8, 72), 1, RANGE)
    # 4. the host call's length, last
    host = lib.dxtlt_untransform_decode_bc6h_images
    good = one(0, 8, 8, DST, 64)
    assert host(SRC, 64 + 3, good, 1) == E_LENGTH and why(lib) == "dxtlt: len is not a multiple of the block size"
    assert host(SRC, 48 + 3, good, 1) == E_ARGUMENT and why(lib) == RANGE                  # the range before the length
    assert host(SRC, 64 + 3, one(0, 8, 8, DST, 63), 1) == E_ARGUMENT and why(lib) == SMALL_PITCH
    assert host(SRC, 64 + 3, one(0, 8, 8, None, 64), 1) == E_ARGUMENT and why(lib) == NULL_PIXELS
    assert host(SRC, 64 + 3, array_of([(0, 8, 8, DST, 64), (0, 8, 8, DST + 4096, 64)]), 2) == E_ARGUMENT and why(lib) == ORDER
    assert host(None, 64 + 3, empty, 3) == OK


def test_format_6_is_still_refused_by_the_generic_and_the_bc7_region_calls(lib):
    good = array_of([(0, 8, 8, DST, 64)])
    assert lib.dxtlt_untransform_decode_images_device(6, SRC, 4, good, 1, 0, False, False, None) == E_ARGUMENT and "format" in why(lib)
    assert lib.dxtlt_decode_images_device(6, SRC, 4, good, 1, None) == E_ARGUMENT and "format" in why(lib)
    assert lib.dxtlt_untransform_decode_images(6, SRC, 64, good, 1, 0, False, False) == E_ARGUMENT and "format" in why(lib)
    assert lib.dxtlt_decode_images_device(6, None, 0, None, 0, None) == E_ARGUMENT           # the format comes first there
    # the BC7 calls have no format argument: they are RGBA8888 calls and stay so -- a BC6H caller's pointer on an 8-byte address
    # with rows of 8 * width bytes is simply a valid list to them, and a four-byte one is to them what it is not to the BC6H calls
    four = array_of([(0, 8, 8, DST + 4, 68)])
    assert lib.dxtlt_debug_plan_bc7_images(4, four, 1, None, 0) == 1
    assert lib.dxtlt_debug_plan_bc6h_images(4, four, 1, None, 0) == -1 and why(lib) == MULTIPLES
    small = array_of([(0, 8, 8, DST, 32)])
    assert lib.dxtlt_debug_plan_bc7_images(4, small, 1, None, 0) == 1
    refused(lib, SRC, 4, small, 1, SMALL_PITCH)


# ---- the plan --------------------------------------------------------------------------------------------------------------
def planned(lib, total, regions, cap=64):
    """the BC6H debug call's records; the BC7 debug call gives the same ones for the same list"""
    arr = region_array(regions, [DST + 0x1000000 * i for i in range(len(regions))], [8 * r[1] for r in regions])
    out = (Launch * cap)()
    n = lib.dxtlt_debug_plan_bc6h_images(total, arr, len(regions), out, cap)
    assert 0 <= n <= cap and all(out[i].reserved == 0 for i in range(n))
    got = [(o.first_region, o.region_count, o.first_granule, o.granule_count, o.tail) for o in out[:n]]
    out7 = (Bc7Launch * cap)()
    n7 = lib.dxtlt_debug_plan_bc7_images(total, arr, len(regions), out7, cap)
    assert n7 == n and got == [(o.first_region, o.region_count, o.first_granule, o.granule_count, o.tail) for o in out7[:n]]
    return got


def test_plan_of_the_chain_and_the_faces(lib):
    # the 256 x 256 nine-level chain: one main launch of 5 granules and one tail launch
    assert planned(lib, TOTAL_256, CHAIN_256) == [(0, 9, 0, 5, 0), (0, 9, 5, 1, 1)] == plan_of(TOTAL_256, CHAIN_256)
    # two faces: sixteen regions, one group, both main granules and the tail part
    assert planned(lib, TOTAL_TWO, TWO_FACES) == [(0, 16, 0, 2, 0), (0, 16, 2, 1, 1)] == plan_of(TOTAL_TWO, TWO_FACES)
    # three faces: two groups, granule 2 in both
    assert [len(g) for _, g in groups_of(THREE_FACES)] == [PER_LAUNCH, 8] and 2 * FACE_BLOCKS // GRANULE == 2
    assert planned(lib, TOTAL_THREE, THREE_FACES) == [(0, 16, 0, 3, 0), (16, 8, 2, 2, 0), (16, 8, 4, 1, 1)]
    assert planned(lib, TOTAL_THREE, THREE_FACES) == plan_of(TOTAL_THREE, THREE_FACES)


@pytest.mark.parametrize("total", [1, 37, 1023, 1024, 1025, 2391, 5463])
def test_plan_of_every_total(lib, total):
    lists = [[(0, 4, 4 * total)], [(total - 1, 1, 1)], [(0, 2, 3), (total - 1, 4, 4)] if total > 1 else [(0, 2, 3)]]
    if total >= 5:
        n1 = (total - 2) // 2
        lists.append([(1, 4 * n1, 3), (2 + n1, 4 * (total - 2 - n1), 2)])      # blocks 0 and 1 + n1 in gaps
    for regions in lists:
        got = planned(lib, total, regions)
        assert got == plan_of(total, regions), (total, regions)
        # these lists all reach the buffer's last block: the tail launch is there exactly when there is a tail part
        assert got[-1][4] == (1 if total % GRANULE else 0) and len(got) == (2 if total > GRANULE and total % GRANULE and regions[0][0] < GRANULE else 1)


def test_plan_at_the_edges_of_the_parts_with_gaps_and_empties(lib):
    # a single region wholly inside the tail part: the tail launch only
    assert planned(lib, TOTAL_256, [CHAIN_256[4]]) == [(0, 1, 5, 1, 1)] == plan_of(TOTAL_256, [CHAIN_256[4]])
    # a range that ends exactly at main_blocks: no tail launch
    assert planned(lib, TOTAL_256, CHAIN_256[:2]) == [(0, 2, 0, 5, 0)] == plan_of(TOTAL_256, CHAIN_256[:2])
    assert planned(lib, 2391, [(2044, 16, 4)]) == [(0, 1, 1, 1, 0)]
    assert planned(lib, 2391, [(2044, 20, 4)]) == [(0, 1, 1, 1, 0), (0, 1, 2, 1, 1)]
    # a group is not split at a gap: blocks 0 and 4000 of the chain's buffer are one launch over granules 0 .. 3
    assert planned(lib, TOTAL_256, [(0, 4, 4), (4000, 4, 4)]) == [(0, 2, 0, 4, 0)]
    # empty regions are no part of a group, wherever their first_block points; the group's index is that of its first real region
    regions = [(2**63, 0, 7), CHAIN_256[0], (2**63, 5, 0), CHAIN_256[2], (5400, 0, 0), CHAIN_256[5]]
    assert planned(lib, TOTAL_256, regions) == [(1, 3, 0, 5, 0), (1, 3, 5, 1, 1)] == plan_of(TOTAL_256, regions)
    assert planned(lib, TOTAL_256, [(2**63, 0, 7)]) == [] and planned(lib, TOTAL_256, []) == []


def test_plan_of_a_range_that_needs_the_split_at_2_to_the_21_granules(lib):
    """arithmetic only: no buffer of this size exists.  One block at the front and one near the end of 5 * 2^20 granules and a tail
    part: three launches over the main part and the tail launch"""
    granules = 5 * (1 << 20)
    total = granules * GRANULE + 7
    regions = [(3, 4, 4), (total - 1, 4, 4)]
    want = [(0, 2, 0, MAX_GRANULES, 0), (0, 2, MAX_GRANULES, MAX_GRANULES, 0), (0, 2, 2 * MAX_GRANULES, 1 << 20, 0),
            (0, 2, granules, 1, 1)]
    assert planned(lib, total, regions) == want == plan_of(total, regions)
    # exactly 2^21 granules are one launch, one more is two
    assert planned(lib, MAX_GRANULES * GRANULE, [(0, 4, 4), (MAX_GRANULES * GRANULE - 1, 4, 4)]) == [(0, 2, 0, MAX_GRANULES, 0)]
    total = (MAX_GRANULES + 1) * GRANULE
    assert planned(lib, total, [(0, 4, 4), (total - 1, 4, 4)]) == [(0, 2, 0, MAX_GRANULES, 0), (0, 2, MAX_GRANULES, 1, 0)]


def test_plan_counts_beyond_the_capacity_and_refuses_what_the_call_refuses(lib):
    arr = region_array(THREE_FACES, [DST + 0x1000000 * i for i in range(24)], [8 * r[1] for r in THREE_FACES])
    assert lib.dxtlt_debug_plan_bc6h_images(TOTAL_THREE, arr, 24, None, 0) == 3
    out = (Launch * 3)()
    out[2].first_region = 77
    assert lib.dxtlt_debug_plan_bc6h_images(TOTAL_THREE, arr, 24, out, 2) == 3 and (out[1].first_region, out[1].first_granule) == (16, 2)
    assert out[2].first_region == 77                                                           # counted, not written
    assert lib.dxtlt_debug_plan_bc6h_images(TOTAL_THREE - 1, arr, 24, out, 2) == -1 and why(lib) == RANGE   # the last region does not fit
    assert lib.dxtlt_debug_plan_bc6h_images(TOTAL_THREE, None, 24, out, 2) == -1 and why(lib) == NULL_REGIONS
    bad = array_of([GOOD[1], GOOD[0]])
    assert lib.dxtlt_debug_plan_bc6h_images(100, bad, 2, out, 2) == -1 and why(lib) == ORDER
    assert lib.dxtlt_debug_plan_bc6h_images(100, array_of([(0, 8, 8, None, 64)]), 1, out, 2) == -1 and why(lib) == NULL_PIXELS
    assert lib.dxtlt_debug_plan_bc6h_images(100, array_of([(0, 8, 8, DST, 56)]), 1, out, 2) == -1 and why(lib) == SMALL_PITCH


# ---- Python and C++ ---------------------------------------------------------------------------------------------------------
def test_python_module_exposes_the_bc6h_region_calls(pkg):
    import numpy as np

    from dxt_lossless_transform_amd import image

    with pytest.raises(TypeError):
        image.decode_bc6h_images(np.zeros(16, np.uint8), [(0, 4, 4)])   # device tensors only
    with pytest.raises(pkg.InvalidLength):
        image.untransform_decode_bc6h_images(np.zeros(17, np.uint8), [(0, 4, 4)])
    with pytest.raises(pkg.DeviceError):
        image.untransform_decode_bc6h_images(np.zeros(16, np.uint8), [(1, 4, 4)])   # the region is not in the buffer
    # a list without a non-empty region needs no device
    outs = image.untransform_decode_bc6h_images(np.zeros(16, np.uint8), [(0, 0, 4), (7, 4, 0)])
    assert [o.size for o in outs] == [0, 0]
    assert image.untransform_decode_bc6h_images(np.zeros(16, np.uint8), []) == []


def test_cpp_wrappers_compile_link_and_check_their_arguments(pkg, tmp_path):
    libdir = os.path.dirname(pkg._lib.lib_path())
    exe = str(tmp_path / "test_cpp_bc6h_images")
    src = os.path.join(ROOT, "tests", "cpp", "test_cpp_bc6h_images.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, src, f"-L{libdir}", "-ldxtlt_gfx950",
                           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
