"""Several images of one buffer (include/dxtlt_image.h), everything that needs no GPU: the region lookup of
csrc/image_regions.h, built for the host, against numpy for every block index of the tables the GPU tests use; the mip-chain
helper against dxtlt_image_mip_level; and every argument check of the three calls in the documented order, on made-up
addresses that are never dereferenced."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from image_regions_common import (BPP, CHAIN_256, CHAIN_260, CUBE, E_ARGUMENT, E_LENGTH, GAPS, OK, PER_LAUNCH, TOTAL_256, TOTAL_260,
                                  Region, blocks_of, load, mip_chain, region_array, region_end)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "image_regions_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "image_regions_shim.cpp")])
    l = C.CDLL(so)
    vp, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
    l.shim_region_of_block.argtypes = [sz, vp, vp, vp, vp, vp, u32, u64, sz, vp, vp, vp, vp]
    l.shim_region_of_block.restype = None
    l.shim_region_of_run.argtypes = [sz, vp, vp, vp, vp, vp, u32, u64, sz, u64, vp, vp, vp]
    l.shim_region_of_run.restype = None
    l.shim_region_table_bytes.restype = sz
    return l


# ---- the lookup --------------------------------------------------------------------------------------------------------
TABLES = {
    "chain 256": CHAIN_256,
    "chain 260 x 136": CHAIN_260,
    "gaps": [r for r in GAPS if r[1] and r[2]],             # the calls drop empty regions before a table is made
    "sixteen": CUBE[:PER_LAUNCH],
    "gaps in front and between": [(7, 36, 8), (40, 5, 7), (44, 1, 1), (100, 260, 8)],
}


def table_arrays(regions, bpp):
    first = np.array([r[0] for r in regions], np.uint64)
    width = np.array([r[1] for r in regions], np.uint32)
    height = np.array([r[2] for r in regions], np.uint32)
    pitch = np.array([bpp * r[1] + 4 * (i % 3) for i, r in enumerate(regions)], np.uint64)
    base = np.array([0x7F0000000000 + 0x1000000 * i + 4 * i for i in range(len(regions))], np.uint64)
    return first, width, height, base, pitch


def numpy_lookup(regions, bpp, base, pitch, b):
    """(region or -1, local block, bx, by, cols, rows, offset, address) of every block index of `b`"""
    region = np.full(b.shape, -1, np.int64)
    for i, r in enumerate(regions):
        region[(b >= r[0]) & (b < region_end(r))] = i
    out = np.zeros((8,) + b.shape, np.int64)
    out[0] = region
    for i, (first, width, height) in enumerate(regions):
        m = region == i
        local = b[m] - first
        bpr = (width + 3) // 4
        by, bx = local // bpr, local % bpr
        offset = by * 4 * int(pitch[i]) + bx * 4 * bpp
        out[1:, m] = [local, bx, by, np.minimum(4, width - 4 * bx), np.minimum(4, height - 4 * by), offset, int(base[i]) + offset]
    return out


@pytest.mark.parametrize("bpp", [4, 1, 2])
@pytest.mark.parametrize("name", list(TABLES))
def test_lookup_of_every_block_index(shim, name, bpp):
    regions = TABLES[name]
    assert 0 < len(regions) <= PER_LAUNCH
    first, width, height, base, pitch = table_arrays(regions, bpp)
    b0 = max(0, regions[0][0] - 3)
    n = region_end(regions[-1]) + 70 - b0                   # some blocks in front of the first region and behind the last
    region, local, address = np.zeros(n, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    place = np.zeros(6 * n, np.uint32)
    shim.shim_region_of_block(len(regions), first.ctypes.data, width.ctypes.data, height.ctypes.data, base.ctypes.data,
                              pitch.ctypes.data, bpp, b0, n, region.ctypes.data, local.ctypes.data, place.ctypes.data, address.ctypes.data)
    want = numpy_lookup(regions, bpp, base, pitch, np.arange(b0, b0 + n, dtype=np.int64))
    place = place.reshape(n, 6).astype(np.int64)
    got = np.stack([region.astype(np.int64), local.astype(np.int64), place[:, 0], place[:, 1], place[:, 2], place[:, 3],
                    place[:, 4] | (place[:, 5] << 32), address.astype(np.int64)])
    assert np.array_equal(got, want)
    assert (want[0] == -1).any() and sorted(set(want[0].tolist()) - {-1}) == list(range(len(regions)))


@pytest.mark.parametrize("run", [64, 128])
@pytest.mark.parametrize("name", list(TABLES))
def test_lookup_of_a_waves_run(shim, name, run):
    """a run of 64 / 128 blocks has a region exactly when every one of its blocks lies in that region"""
    regions = TABLES[name]
    first, width, height, base, pitch = table_arrays(regions, 4)
    b0 = max(0, regions[0][0] - 3)
    n = region_end(regions[-1]) + 70 - b0
    region, local, address = np.zeros(n, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    shim.shim_region_of_run(len(regions), first.ctypes.data, width.ctypes.data, height.ctypes.data, base.ctypes.data, pitch.ctypes.data,
                            4, b0, n, run, region.ctypes.data, local.ctypes.data, address.ctypes.data)
    b = np.arange(b0, b0 + n, dtype=np.int64)
    lo, hi = numpy_lookup(regions, 4, base, pitch, b), numpy_lookup(regions, 4, base, pitch, b + run - 1)
    whole = (lo[0] >= 0) & (lo[0] == hi[0])                 # regions ascend: first and last block in one region = all of them
    assert np.array_equal(region, np.where(whole, lo[0], -1))
    assert np.array_equal(local.astype(np.int64), np.where(whole, lo[1], 0))
    assert np.array_equal(address, np.where(whole, base[np.maximum(lo[0], 0)], 0).astype(np.uint64))


def test_lookup_wraps_safely_at_the_top_of_the_block_range(shim):
    regions = [(2**64 - 100, 40, 40)]                       # 100 blocks: the region ends at 2^64 exactly
    first, width, height, base, pitch = table_arrays(regions, 4)
    n = 130
    region, local, address = np.zeros(n, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    place = np.zeros(6 * n, np.uint32)
    shim.shim_region_of_block(1, first.ctypes.data, width.ctypes.data, height.ctypes.data, base.ctypes.data, pitch.ctypes.data, 4,
                              2**64 - 110, n, region.ctypes.data, local.ctypes.data, place.ctypes.data, address.ctypes.data)
    # blocks 2^64 - 110 .. 2^64 - 101: none; the region's 100; then indices 0 .. 19 after the wrap: none
    assert region.tolist() == [-1] * 10 + [0] * 100 + [-1] * 20
    assert local[10:110].tolist() == list(range(100))


def test_table_fits_the_kernel_arguments(shim):
    assert shim.shim_regions_per_launch() == PER_LAUNCH
    assert shim.shim_region_table_bytes() <= 1024


# ---- the mip chain helper ----------------------------------------------------------------------------------------------
def chain_of(lib, width, height, mip_count, first):
    arr = (Region * mip_count)()
    for r in arr:
        r.pixels, r.pitch = 0x1234560, 0x777
    total = C.c_uint64()
    assert lib.dxtlt_image_mip_chain(width, height, mip_count, first, arr, C.byref(total)) == OK
    assert all(r.pixels == 0x1234560 and r.pitch == 0x777 for r in arr), "pixels and pitch are the caller's"
    return [(r.first_block, r.width, r.height) for r in arr], total.value


@pytest.mark.parametrize("width,height,mip_count", [(256, 256, 9), (260, 136, 9), (1, 1, 1), (5, 7, 3), (1026, 9, 11), (8, 2, 6),
                                                    (8, 8, 40), (16384, 16384, 15)])
@pytest.mark.parametrize("first", [0, 341, 2**40 + 5])
def test_mip_chain_agrees_with_mip_level_level_by_level(lib, width, height, mip_count, first):
    levels, end = chain_of(lib, width, height, mip_count, first)
    assert (levels, end) == mip_chain(width, height, mip_count, first)
    for k in range(mip_count):
        w, h = C.c_uint32(), C.c_uint32()
        at, num, total = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert lib.dxtlt_image_mip_level(width, height, mip_count, k, C.byref(w), C.byref(h), C.byref(at), C.byref(num), C.byref(total)) == OK
        assert levels[k] == (first + at.value, w.value, h.value) and end == first + total.value
        assert num.value == blocks_of(w.value, h.value)


def test_mip_chain_worked_vector_and_errors(lib):
    levels, total = chain_of(lib, 256, 256, 9, 0)
    assert total == 5463 and [levels[k][0] for k in (1, 3, 7, 8)] == [4096, 5376, 5461, 5462]
    assert (levels, total) == (CHAIN_256, TOTAL_256)
    assert chain_of(lib, 260, 136, 9, 0) == (CHAIN_260, TOTAL_260)
    arr = (Region * 9)()
    assert lib.dxtlt_image_mip_chain(256, 256, 9, 0, arr, None) == OK          # the total may be NULL
    assert lib.dxtlt_image_mip_chain(0, 256, 9, 0, arr, None) == E_ARGUMENT
    assert lib.dxtlt_image_mip_chain(256, 0, 9, 0, arr, None) == E_ARGUMENT
    assert lib.dxtlt_image_mip_chain(256, 256, 0, 0, arr, None) == E_ARGUMENT
    assert lib.dxtlt_image_mip_chain(256, 256, 9, 0, None, None) == E_ARGUMENT


def test_python_mip_chain(pkg):
    from dxt_lossless_transform_amd import image

    assert image.mip_chain(256, 256, 9) == (CHAIN_256, TOTAL_256)
    assert image.mip_chain(64, 64, 5, 341) == (CUBE[5:10], 682)
    for k, (first, w, h) in enumerate(image.mip_chain(260, 136, 9, 11)[0]):
        lw, lh, lfirst, _, _ = image.mip_level(260, 136, 9, k)
        assert (first, w, h) == (11 + lfirst, lw, lh)
    with pytest.raises(pkg.DeviceError):
        image.mip_chain(0, 4, 1)


# ---- argument checks: none of these may touch a device or an address ---------------------------------------------------
SRC, DST = 0x7F1000000000, 0x7F2000000000   # made up


def calls(lib, fmt, src, total, arr, count, mode=1, sa=True, sc=True):
    """the status of the three calls for one argument set (the host call with len = total blocks)"""
    bs = 8 if fmt in (1, 4) else 16
    return (lib.dxtlt_untransform_decode_images_device(fmt, src, total, arr, count, mode, sa, sc, None),
            lib.dxtlt_decode_images_device(fmt, src, total, arr, count, None),
            lib.dxtlt_untransform_decode_images(fmt, src, total * bs, arr, count, mode, sa, sc))


def one(first, width, height, pixels, pitch):
    return region_array([(first, width, height)], [pixels], [pitch])


@pytest.mark.parametrize("fmt", [1, 2, 3, 4, 5])
def test_every_argument_check_in_the_documented_order(lib, fmt):
    bpp = BPP["bc%d" % fmt]
    bs = 8 if fmt in (1, 4) else 16
    row = 8 * bpp                                            # an 8 x 8 image: 4 blocks
    good = one(0, 8, 8, DST, row)
    bad_everywhere = one(2**64 - 2, 8, 8, None, 1)           # NULL pixels, a small pitch, a range that wraps
    # 1. the format comes first
    for f in (0, 6, -1, 7):
        assert calls(lib, f, None, 0, None, 1) == (E_ARGUMENT,) * 3
    # 2. no regions, or only empty ones: OK whatever else is passed -- NULL buffer, bad mode, a length that is no multiple
    assert calls(lib, fmt, None, 0, None, 0, mode=9) == (OK,) * 3
    assert calls(lib, fmt, None, 0, good, 0, mode=9) == (OK,) * 3
    empty = region_array([(2**64 - 1, 0, 8), (5, 8, 0), (0, 0, 0)], [None, 1, DST], [0, 1, 3])
    assert calls(lib, fmt, None, 0, empty, 3, mode=9) == (OK,) * 3
    assert lib.dxtlt_untransform_decode_images(fmt, None, 3, empty, 3, 9, True, True) == OK
    # 3. a NULL buffer or regions pointer, before anything about a region
    assert calls(lib, fmt, None, 4, bad_everywhere, 1) == (E_ARGUMENT,) * 3
    assert calls(lib, fmt, SRC, 4, None, 1) == (E_ARGUMENT,) * 3
    assert calls(lib, fmt, None, 4, good, 1) == (E_ARGUMENT,) * 3
    # 4. per region: NULL pixels, the pitch, the alignment, the range, the order
    assert calls(lib, fmt, SRC, 4, one(0, 8, 8, None, row), 1) == (E_ARGUMENT,) * 3
    assert calls(lib, fmt, SRC, 4, one(0, 8, 8, DST, row - bpp), 1) == (E_ARGUMENT,) * 3
    assert calls(lib, fmt, SRC, 2**40, one(0, 0x40000001, 1, DST, 4 * bpp), 1) == (E_ARGUMENT,) * 3   # bpp * width needs 33 bits
    if fmt <= 3:
        for pixels, pitch in ((DST + 2, row), (DST + 1, row), (DST, row + 2), (DST, row + 1)):
            assert calls(lib, fmt, SRC, 4, one(0, 8, 8, pixels, pitch), 1) == (E_ARGUMENT,) * 3
    if fmt == 5:
        for pixels, pitch in ((DST + 1, row), (DST, row + 1)):
            assert calls(lib, fmt, SRC, 4, one(0, 8, 8, pixels, pitch), 1) == (E_ARGUMENT,) * 3
    assert calls(lib, fmt, SRC, 3, good, 1) == (E_ARGUMENT,) * 3                                    # 4 blocks of 3
    assert calls(lib, fmt, SRC, 4, one(1, 8, 8, DST, row), 1) == (E_ARGUMENT,) * 3
    assert calls(lib, fmt, SRC, 100, one(97, 8, 8, DST, row), 1) == (E_ARGUMENT,) * 3
    assert calls(lib, fmt, SRC, 100, one(2**64 - 2, 8, 8, DST, row), 1) == (E_ARGUMENT,) * 3         # first_block + blocks wraps
    assert calls(lib, fmt, SRC, 2**64 - 1, one(2**64 - 2, 8, 8, DST, row), 1) == (E_ARGUMENT,) * 3
    two = lambda a, b: region_array([(a, 8, 8), (b, 8, 8)], [DST, DST + 4096], [row, row])
    assert calls(lib, fmt, SRC, 100, two(0, 3), 2) == (E_ARGUMENT,) * 3                              # overlap: blocks 0..3 and 3..6
    assert calls(lib, fmt, SRC, 100, two(10, 2), 2) == (E_ARGUMENT,) * 3                             # descending
    assert calls(lib, fmt, SRC, 100, two(10, 10), 2) == (E_ARGUMENT,) * 3                            # the same range twice
    # an empty region between two others is skipped, whatever it holds: the overlap of the two around it is still found
    three = region_array([(10, 8, 8), (2**64 - 1, 0, 0), (12, 8, 8)], [DST, None, DST + 4096], [row, 0, row])
    assert calls(lib, fmt, SRC, 100, three, 3) == (E_ARGUMENT,) * 3
    # 5. the decorrelation mode, for formats 1 - 3, behind the regions; 6. the host call's length, last
    if fmt <= 3:
        assert lib.dxtlt_untransform_decode_images_device(fmt, SRC, 4, good, 1, 4, True, True, None) == E_ARGUMENT
        assert lib.dxtlt_untransform_decode_images_device(fmt, SRC, 4, good, 1, 255, True, True, None) == E_ARGUMENT
        assert lib.dxtlt_untransform_decode_images(fmt, SRC, 4 * bs, good, 1, 4, True, True) == E_ARGUMENT
        assert lib.dxtlt_untransform_decode_images(fmt, SRC, 4 * bs + 3, good, 1, 4, True, True) == E_ARGUMENT   # the mode before the length
    assert lib.dxtlt_untransform_decode_images(fmt, SRC, 4 * bs + 3, good, 1, 1, True, True) == E_LENGTH
    assert lib.dxtlt_untransform_decode_images(fmt, SRC, 3 * bs + 3, good, 1, 1, True, True) == E_ARGUMENT       # the range before the length
    if fmt >= 4:   # the mode is ignored: with 4 the call gets as far as the length check
        assert lib.dxtlt_untransform_decode_images(fmt, SRC, 4 * bs + 3, good, 1, 4, True, True) == E_LENGTH


def test_decorrelation_mode_4_is_refused_for_bc3_and_ignored_for_bc4(lib):
    """the one check whose verdict depends on the format: the same arguments, refused as an argument for format 3, while format 4
    ignores the mode and goes on to the next check (here the host call's length)"""
    bc3 = one(0, 8, 8, DST, 32)
    bc4 = one(0, 8, 8, DST, 8)
    assert lib.dxtlt_untransform_decode_images(3, SRC, 4 * 16 + 1, bc3, 1, 4, True, True) == E_ARGUMENT
    assert lib.dxtlt_untransform_decode_images(4, SRC, 4 * 8 + 1, bc4, 1, 4, True, True) == E_LENGTH
    assert lib.dxtlt_untransform_decode_images_device(3, SRC, 4, bc3, 1, 4, True, True, None) == E_ARGUMENT
