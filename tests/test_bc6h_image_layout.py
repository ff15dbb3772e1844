"""BC6H image decoders (include/dxtlt_bc6h_image.h), everything that needs no GPU: every argument check of the three image calls,
in the documented order, on made-up addresses that are never dereferenced; the RGBA, region and BC7 calls still refuse BC6H; and
the Python surface's length errors."""
import ctypes as C

import numpy as np
import pytest

OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
SRC, DST = 0x7F1000000000, 0x7F2000000000   # made up


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, i32, u32, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
    l.dxtlt_decode_bc6h_image_device.argtypes = [vp, u32, u32, vp, u64, vp]
    l.dxtlt_untransform_decode_bc6h_image_device.argtypes = [vp, u64, u64, u32, u32, vp, u64, vp]
    l.dxtlt_untransform_decode_bc6h_image.argtypes = [vp, C.c_size_t, u64, u32, u32, vp, u64]
    for f in (l.dxtlt_decode_bc6h_image_device, l.dxtlt_untransform_decode_bc6h_image_device, l.dxtlt_untransform_decode_bc6h_image):
        f.restype = i32
    l.dxtlt_last_error.restype = C.c_char_p
    return l


def why(lib):
    return lib.dxtlt_last_error().decode()


def test_every_argument_error_of_the_device_pointer_calls(lib):
    dec, fused = lib.dxtlt_decode_bc6h_image_device, lib.dxtlt_untransform_decode_bc6h_image_device
    # 1: empty images do nothing, whatever else is passed
    assert dec(None, 0, 8, None, 0, None) == OK
    assert dec(None, 8, 0, None, 3, None) == OK
    assert fused(None, 0, 5, 0, 8, None, 1, None) == OK
    assert fused(None, 0, 2**64 - 2, 8, 0, None, 1, None) == OK
    # 2: NULL pointers -- before the pitch
    assert dec(None, 8, 8, DST, 64, None) == E_ARGUMENT
    assert dec(SRC, 8, 8, None, 64, None) == E_ARGUMENT
    assert fused(None, 4, 0, 8, 8, DST, 64, None) == E_ARGUMENT
    assert fused(SRC, 4, 0, 8, 8, None, 63, None) == E_ARGUMENT and "NULL" in why(lib)
    # 3: pitch < 8 * width (also for a width whose 8 * width needs more than 32 bits) -- before the multiples
    assert dec(SRC, 8, 8, DST, 56, None) == E_ARGUMENT
    assert dec(SRC, 8, 8, DST, 32, None) == E_ARGUMENT and "smaller" in why(lib)          # an RGBA8888 pitch is too small
    assert dec(SRC, 0xFFFFFFFF, 1, DST, 0x7FFFFFFF0, None) == E_ARGUMENT and "smaller" in why(lib)
    assert fused(SRC, 4, 0, 8, 8, DST + 1, 60, None) == E_ARGUMENT and "smaller" in why(lib)
    # 4: pitch and the pixel pointer are multiples of 8 -- before the range
    assert dec(SRC, 8, 8, DST, 68, None) == E_ARGUMENT and "multiples" in why(lib)
    assert dec(SRC, 8, 8, DST + 4, 64, None) == E_ARGUMENT and "multiples" in why(lib)
    assert fused(SRC, 3, 0, 8, 8, DST, 66, None) == E_ARGUMENT and "multiples" in why(lib)
    assert fused(SRC, 3, 0, 8, 8, DST + 4, 64, None) == E_ARGUMENT and "multiples" in why(lib)
    # 5: the range -- an 8 x 8 image is 4 blocks
    assert fused(SRC, 3, 0, 8, 8, DST, 64, None) == E_ARGUMENT and "total_blocks" in why(lib)
    assert fused(SRC, 4, 1, 8, 8, DST, 64, None) == E_ARGUMENT
    assert fused(SRC, 100, 97, 8, 8, DST, 64, None) == E_ARGUMENT
    assert fused(SRC, 100, 101, 8, 8, DST, 64, None) == E_ARGUMENT
    assert fused(SRC, 100, 2**64 - 2, 8, 8, DST, 64, None) == E_ARGUMENT and "total_blocks" in why(lib)   # wraps
    # the block pointer may have any alignment: an odd one gets as far as the range
    assert fused(SRC + 1, 3, 0, 8, 8, DST + 8, 72, None) == E_ARGUMENT and "total_blocks" in why(lib)


def test_every_argument_error_of_the_host_pointer_call(lib):
    host = lib.dxtlt_untransform_decode_bc6h_image
    assert host(None, 0, 0, 0, 8, None, 0) == OK
    assert host(None, 3, 7, 8, 0, None, 0) == OK
    assert host(None, 64, 0, 8, 8, DST, 64) == E_ARGUMENT
    assert host(SRC, 64, 0, 8, 8, None, 64) == E_ARGUMENT and "NULL" in why(lib)
    assert host(SRC, 64, 0, 8, 8, DST, 63) == E_ARGUMENT and "smaller" in why(lib)
    assert host(SRC, 64, 0, 8, 8, DST, 68) == E_ARGUMENT and "multiples" in why(lib)
    assert host(SRC, 64, 0, 8, 8, DST + 4, 64) == E_ARGUMENT and "multiples" in why(lib)
    assert host(SRC, 48, 0, 8, 8, DST, 64) == E_ARGUMENT and "total_blocks" in why(lib)
    assert host(SRC, 64, 1, 8, 8, DST, 64) == E_ARGUMENT
    assert host(SRC, 64, 2**64 - 2, 8, 8, DST, 64) == E_ARGUMENT and "total_blocks" in why(lib)   # wraps
    # 6: len not a multiple of 16 is the LAST check: a range that does not fit either is the argument error
    assert host(SRC, 64 + 3, 0, 8, 8, DST, 64) == E_LENGTH
    assert host(SRC, 48 + 3, 0, 8, 8, DST, 64) == E_ARGUMENT
    assert host(SRC, 64 + 3, 0, 8, 8, DST, 63) == E_ARGUMENT
    assert host(SRC, 64 + 3, 0, 8, 8, DST + 1, 64) == E_ARGUMENT


def test_the_rgba_region_and_bc7_calls_still_refuse_bc6h(lib):
    vp, i32, u32, u64, u8, b = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint8, C.c_bool
    lib.dxtlt_decode_image_device.argtypes = [i32, vp, u32, u32, vp, u64, vp]
    lib.dxtlt_untransform_decode_image_device.argtypes = [i32, vp, u64, u64, u32, u32, u8, b, b, vp, u64, vp]
    lib.dxtlt_decode_images_device.argtypes = [i32, vp, u64, vp, C.c_size_t, vp]
    lib.dxtlt_decode_channel_image_device.argtypes = [i32, vp, u32, u32, vp, u64, vp]
    for f in (lib.dxtlt_decode_image_device, lib.dxtlt_untransform_decode_image_device, lib.dxtlt_decode_images_device,
              lib.dxtlt_decode_channel_image_device):
        f.restype = i32
    assert lib.dxtlt_decode_image_device(6, SRC, 8, 8, DST, 64, None) == E_ARGUMENT
    assert lib.dxtlt_untransform_decode_image_device(6, SRC, 4, 0, 8, 8, 0, False, False, DST, 64, None) == E_ARGUMENT
    assert lib.dxtlt_decode_images_device(6, SRC, 4, None, 0, None) == E_ARGUMENT
    assert lib.dxtlt_decode_channel_image_device(6, SRC, 8, 8, DST, 64, None) == E_ARGUMENT


def test_python_module_exposes_the_bc6h_calls(pkg):
    from dxt_lossless_transform_amd import decode, image

    assert callable(image.decode_bc6h_image) and callable(image.untransform_decode_bc6h_image) and callable(decode.decode_bc6h_blocks)
    with pytest.raises(TypeError):
        image.decode_bc6h_image(np.zeros(16, np.uint8), 4, 4)   # device tensors only
    with pytest.raises(pkg.InvalidLength):
        image.untransform_decode_bc6h_image(np.zeros(17, np.uint8), 4, 4)
    with pytest.raises(pkg.InvalidLength):
        image.untransform_decode_bc6h_image(np.zeros(32, np.uint8), 4, 4, total_blocks=3)
    with pytest.raises(pkg.OutputBufferTooSmall):
        image.untransform_decode_bc6h_image(np.zeros(16, np.uint8), 4, 4, out=np.zeros(127, np.uint8))   # 4 rows of 32 bytes
    # an empty image needs no device; the default pitch is 8 bytes per pixel
    assert image.untransform_decode_bc6h_image(np.zeros(16, np.uint8), 0, 4).size == 0
