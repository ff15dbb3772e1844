"""Image decoders (include/dxtlt_image.h), everything that needs no GPU: the mip-level arithmetic against a short Python
statement, the image sink (csrc/image_sink.h, built for the host) against numpy -- the pixels it addresses are exactly the
row-major image -- and every argument check of the three calls, on made-up addresses that are never dereferenced."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
# the shapes of tests/test_image_gpu.py
SHAPES = [(1, 1), (2, 3), (4, 4), (5, 7), (20, 9), (256, 4), (260, 8), (1026, 9), (1024, 8)]


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, i32, u32, u64, u8, b = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint8, C.c_bool
    l.dxtlt_decode_image_device.argtypes = [i32, vp, u32, u32, vp, u64, vp]
    l.dxtlt_untransform_decode_image_device.argtypes = [i32, vp, u64, u64, u32, u32, u8, b, b, vp, u64, vp]
    l.dxtlt_untransform_decode_image.argtypes = [i32, vp, C.c_size_t, u64, u32, u32, u8, b, b, vp, u64]
    l.dxtlt_image_mip_level.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64),
                                        C.POINTER(u64)]
    for f in (l.dxtlt_decode_image_device, l.dxtlt_untransform_decode_image_device, l.dxtlt_untransform_decode_image,
              l.dxtlt_image_mip_level):
        f.restype = i32
    return l


# ---- mip levels ------------------------------------------------------------------------------------------------------
def mip_chain(width, height, mip_count):
    """[(level width, level height, first block, blocks)] and the total"""
    levels, first = [], 0
    for k in range(mip_count):
        w, h = max(1, width >> k), max(1, height >> k)
        blocks = ((w + 3) // 4) * ((h + 3) // 4)
        levels.append((w, h, first, blocks))
        first += blocks
    return levels, first


def mip_level(lib, width, height, mip_count, level):
    w, h = C.c_uint32(), C.c_uint32()
    first, num, total = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = lib.dxtlt_image_mip_level(width, height, mip_count, level, C.byref(w), C.byref(h), C.byref(first), C.byref(num), C.byref(total))
    return rc, (w.value, h.value, first.value, num.value), total.value


@pytest.mark.parametrize("width,height,mip_count", [(256, 256, 9), (1026, 9, 11), (1, 1, 1), (5, 7, 3)])
def test_mip_level_matches_the_python_statement(lib, width, height, mip_count):
    levels, total = mip_chain(width, height, mip_count)
    for k, want in enumerate(levels):
        assert mip_level(lib, width, height, mip_count, k) == (OK, want, total), k


def test_mip_level_worked_vector(lib):
    assert mip_level(lib, 256, 256, 9, 1) == (OK, (128, 128, 4096, 1024), 5463)
    assert mip_level(lib, 256, 256, 9, 3) == (OK, (32, 32, 5376, 64), 5463)
    assert mip_level(lib, 256, 256, 9, 7) == (OK, (2, 2, 5461, 1), 5463)
    assert mip_level(lib, 256, 256, 9, 8) == (OK, (1, 1, 5462, 1), 5463)


def test_mip_level_errors_and_null_outputs(lib):
    assert mip_level(lib, 256, 256, 9, 9)[0] == E_ARGUMENT       # level >= mip_count
    assert mip_level(lib, 256, 256, 0, 0)[0] == E_ARGUMENT       # no levels
    assert mip_level(lib, 0, 256, 9, 0)[0] == E_ARGUMENT
    assert mip_level(lib, 256, 0, 9, 0)[0] == E_ARGUMENT
    assert lib.dxtlt_image_mip_level(256, 256, 9, 1, None, None, None, None, None) == OK
    # levels past the 32nd are 1 x 1 like every level since the dimensions ran out
    levels, total = mip_chain(8, 8, 40)
    assert mip_level(lib, 8, 8, 40, 39) == (OK, levels[39], total)
    assert mip_level(lib, 8, 8, 40, 33) == (OK, levels[33], total)


# ---- the sink --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sink(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "image_sink_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "image_sink_shim.cpp")])
    l = C.CDLL(so)
    l.shim_image_sink_pixels.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    l.shim_image_sink_pixels.restype = C.c_size_t
    l.shim_image_sink_place.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]
    l.shim_image_sink_place.restype = None
    l.shim_image_blocks.argtypes = [C.c_uint32, C.c_uint32]
    l.shim_image_blocks.restype = C.c_uint64
    return l


@pytest.mark.parametrize("width,height", SHAPES)
@pytest.mark.parametrize("extra_pitch", [0, 20])
def test_sink_addresses_are_exactly_the_row_major_image(sink, width, height, extra_pitch):
    base, pitch = 0x7F0000001000, 4 * width + extra_pitch
    bpr = (width + 3) // 4
    assert sink.shim_image_blocks(width, height) == bpr * ((height + 3) // 4)
    cap = width * height + 64
    address, block, pixel = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
    n = sink.shim_image_sink_pixels(base, pitch, width, height, address.ctypes.data, block.ctypes.data, pixel.ctypes.data, cap)
    assert n == width * height   # every pixel once at most: clipped pixels absent
    got = {(int(a), int(b), int(p)) for a, b, p in zip(address[:n], block[:n], pixel[:n])}
    y, x = np.mgrid[0:height, 0:width]
    want = {(int(a), int(b), int(p)) for a, b, p in zip((base + y * pitch + 4 * x).ravel(), ((y // 4) * bpr + x // 4).ravel(),
                                                        ((y % 4) * 4 + x % 4).ravel())}
    assert len(want) == n and got == want   # no address outside a row, none twice, the right pixel of the right block at each


def test_sink_clip_masks(sink):
    out = (C.c_uint32 * 4)()

    def place(width, height, b):
        sink.shim_image_sink_place(4 * width, width, height, b, out)
        return tuple(out)

    assert place(1026, 9, 0) == (0, 0, 4, 4)
    assert place(1026, 9, 256) == (256, 0, 2, 4)      # last column: 2 pixels wide
    assert place(1026, 9, 257) == (0, 1, 4, 4)
    assert place(1026, 9, 2 * 257 + 5) == (5, 2, 4, 1)   # last row: 1 pixel high
    assert place(1026, 9, 770) == (256, 2, 2, 1)
    assert place(1, 1, 0) == (0, 0, 1, 1)
    assert place(5, 7, 3) == (1, 1, 1, 3)


@pytest.mark.parametrize("width", [20, 18])
@pytest.mark.parametrize("pitch,height", [(2**30 + 48, 9), (2**32 + 48, 2), (2**30 + 47, 9), (2**32 + 47, 2)])
def test_sink_offsets_beyond_32_bits(sink, pitch, height, width):
    """The pitches of tests/test_wide_offsets_gpu.py: 4 * by * pitch passes 2^32 at block row 1 of a 20 x 9 image, and a pitch
    of 2^32 + 48 does not fit 32 bits itself.  Every pixel address against y * pitch + 4 * x in Python integers, and the clip
    of the last row (and, at width 18, of the last column)."""
    base = 0x7F0000001000
    blocks = 5 * ((height + 3) // 4)
    assert sink.shim_image_blocks(width, height) == blocks
    cap = width * height
    address, block, pixel = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
    n = sink.shim_image_sink_pixels(base, pitch, width, height, address.ctypes.data, block.ctypes.data, pixel.ctypes.data, cap)
    assert n == cap
    got = sorted((int(a), int(b), int(p)) for a, b, p in zip(address, block, pixel))
    want = sorted((base + y * pitch + 4 * x, (y // 4) * 5 + x // 4, (y % 4) * 4 + x % 4) for y in range(height) for x in range(width))
    assert got == want
    assert max(a for a, _, _ in want) - base >= 2**32   # the case is what it says
    out = (C.c_uint32 * 4)()
    for b in range(blocks):
        sink.shim_image_sink_place(pitch, width, height, b, out)
        bx, by = b % 5, b // 5
        assert tuple(out) == (bx, by, min(4, width - 4 * bx), min(4, height - 4 * by)), b


# ---- argument checks: none of these may touch a device or an address ---------------------------------------------------
SRC, DST = 0x7F1000000000, 0x7F2000000000   # made up


def test_every_argument_error_of_the_device_pointer_calls(lib):
    dec, fused = lib.dxtlt_decode_image_device, lib.dxtlt_untransform_decode_image_device
    for fmt in (0, 4, 7, -1):
        assert dec(fmt, SRC, 8, 8, DST, 32, None) == E_ARGUMENT
        assert fused(fmt, SRC, 4, 0, 8, 8, 1, True, True, DST, 32, None) == E_ARGUMENT
    for fmt in (1, 2, 3):
        # empty images do nothing, whatever else is passed
        assert dec(fmt, None, 0, 8, None, 0, None) == OK
        assert dec(fmt, None, 8, 0, None, 0, None) == OK
        assert fused(fmt, None, 0, 0, 0, 8, 1, True, True, None, 0, None) == OK
        assert fused(fmt, None, 0, 0, 8, 0, 1, True, True, None, 0, None) == OK
        # NULL pointers
        assert dec(fmt, None, 8, 8, DST, 32, None) == E_ARGUMENT
        assert dec(fmt, SRC, 8, 8, None, 32, None) == E_ARGUMENT
        assert fused(fmt, None, 4, 0, 8, 8, 1, True, True, DST, 32, None) == E_ARGUMENT
        assert fused(fmt, SRC, 4, 0, 8, 8, 1, True, True, None, 32, None) == E_ARGUMENT
        # pitch < 4 * width (also for a width whose 4 * width needs more than 32 bits)
        assert dec(fmt, SRC, 8, 8, DST, 28, None) == E_ARGUMENT
        assert dec(fmt, SRC, 0x40000001, 1, DST, 4, None) == E_ARGUMENT
        assert fused(fmt, SRC, 4, 0, 8, 8, 1, True, True, DST, 28, None) == E_ARGUMENT
        # pitch or pixel pointer not a multiple of 4
        assert dec(fmt, SRC, 8, 8, DST, 34, None) == E_ARGUMENT
        assert dec(fmt, SRC, 8, 8, DST + 2, 32, None) == E_ARGUMENT
        assert fused(fmt, SRC, 4, 0, 8, 8, 1, True, True, DST, 33, None) == E_ARGUMENT
        assert fused(fmt, SRC, 4, 0, 8, 8, 1, True, True, DST + 1, 32, None) == E_ARGUMENT
        # decorrelation mode
        assert fused(fmt, SRC, 4, 0, 8, 8, 4, True, True, DST, 32, None) == E_ARGUMENT
        assert fused(fmt, SRC, 4, 0, 8, 8, 255, True, True, DST, 32, None) == E_ARGUMENT
        # the range: an 8 x 8 image is 4 blocks
        assert fused(fmt, SRC, 3, 0, 8, 8, 1, True, True, DST, 32, None) == E_ARGUMENT
        assert fused(fmt, SRC, 4, 1, 8, 8, 1, True, True, DST, 32, None) == E_ARGUMENT
        assert fused(fmt, SRC, 100, 97, 8, 8, 1, True, True, DST, 32, None) == E_ARGUMENT
        assert fused(fmt, SRC, 100, 2**64 - 2, 8, 8, 1, True, True, DST, 32, None) == E_ARGUMENT   # first + blocks wraps


def test_every_argument_error_of_the_host_pointer_call(lib):
    host = lib.dxtlt_untransform_decode_image
    assert host(0, SRC, 64, 0, 8, 8, 1, True, True, DST, 32) == E_ARGUMENT
    assert host(4, SRC, 64, 0, 8, 8, 1, True, True, DST, 32) == E_ARGUMENT
    for fmt, bs in ((1, 8), (2, 16), (3, 16)):
        assert host(fmt, None, 0, 0, 0, 8, 1, True, True, None, 0) == OK
        assert host(fmt, None, 0, 0, 8, 0, 1, True, True, None, 0) == OK
        assert host(fmt, None, 4 * bs, 0, 8, 8, 1, True, True, DST, 32) == E_ARGUMENT
        assert host(fmt, SRC, 4 * bs, 0, 8, 8, 1, True, True, None, 32) == E_ARGUMENT
        assert host(fmt, SRC, 4 * bs, 0, 8, 8, 1, True, True, DST, 28) == E_ARGUMENT
        assert host(fmt, SRC, 4 * bs, 0, 8, 8, 1, True, True, DST, 34) == E_ARGUMENT
        assert host(fmt, SRC, 4 * bs, 0, 8, 8, 1, True, True, DST + 2, 32) == E_ARGUMENT
        assert host(fmt, SRC, 4 * bs, 0, 8, 8, 4, True, True, DST, 32) == E_ARGUMENT
        assert host(fmt, SRC, 3 * bs, 0, 8, 8, 1, True, True, DST, 32) == E_ARGUMENT
        assert host(fmt, SRC, 4 * bs, 1, 8, 8, 1, True, True, DST, 32) == E_ARGUMENT
        # len not a multiple of the block size: the last check, so a range that does not fit either is the argument error
        assert host(fmt, SRC, 4 * bs + 3, 0, 8, 8, 1, True, True, DST, 32) == E_LENGTH
        assert host(fmt, SRC, 3 * bs + 3, 0, 8, 8, 1, True, True, DST, 32) == E_ARGUMENT
        assert host(fmt, SRC, 4 * bs + 3, 0, 8, 8, 7, True, True, DST, 32) == E_ARGUMENT


def test_python_module_is_part_of_the_package(pkg):
    from dxt_lossless_transform_amd import image

    assert image.mip_level(256, 256, 9, 3) == (32, 32, 5376, 64, 5463)
    assert image.image_blocks(1026, 9) == 771
    with pytest.raises(pkg.DeviceError):
        image.mip_level(256, 256, 9, 9)
