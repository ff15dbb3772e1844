"""Uncompressed pixels (RGBA8888 / BGRA8888 / BGR888, docs/PIXEL_FORMAT.md) without a device: the CPU statement against the
document's worked vectors and itself, the tagged header words, and what the C calls decide before any device work."""
import ctypes as C
import struct

import numpy as np
import pytest

import pixels_ref as R

COUNTS = list(range(0, 131)) + [4095, 4096, 4097, 8191, 8192, 8193, 12_411]
OK, E_LENGTH, E_ARGUMENT, E_NO_DEVICE = 0, 1, 2, 3
FF_OK, FF_TOO_SMALL, FF_UNKNOWN, FF_CORRUPTED, FF_ALIGNMENT = 0, 1, 4, 5, 6


def pixels(P, B, seed):
    return np.random.default_rng(seed).integers(0, 256, P * B, dtype=np.uint8)


# ---- the CPU statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(R.VECTOR_OUTPUT))
def test_worked_vectors(key):
    B, decorrelate, layout = key
    x = np.frombuffer(R.VECTOR_INPUT[B], dtype=np.uint8)
    y = R.forward(x, B, decorrelate, layout)
    assert y.tobytes() == R.VECTOR_OUTPUT[key]
    assert R.inverse(y, B, decorrelate, layout).tobytes() == R.VECTOR_INPUT[B]


@pytest.mark.parametrize("decorrelate,layout", R.SETTINGS)
@pytest.mark.parametrize("B", [3, 4])
def test_round_trip_at_every_count(B, decorrelate, layout):
    for P in COUNTS:
        x = pixels(P, B, 1000 * B + P)
        y = R.forward(x, B, decorrelate, layout)
        assert y.size == x.size
        assert np.array_equal(R.inverse(y, B, decorrelate, layout), x), P


@pytest.mark.parametrize("B", [3, 4])
def test_segments_are_independent(B):
    P = 2 * R.SEGMENT + 17
    x = pixels(P, B, 7)
    y = R.forward(x, B, True, R.PLANAR_DELTA).reshape(B, P)
    for pixel in (0, 100, R.SEGMENT - 1):            # one byte of segment 0 at a time, its last byte included
        x2 = x.copy()
        x2[pixel * B + 1] ^= 0x5A                    # G: reaches planes 0, 1 and 2
        y2 = R.forward(x2, B, True, R.PLANAR_DELTA).reshape(B, P)
        assert not np.array_equal(y2[:, :R.SEGMENT], y[:, :R.SEGMENT])
        assert np.array_equal(y2[:, R.SEGMENT:], y[:, R.SEGMENT:])


def test_rgba_and_bgra_are_one_transform():
    """byte 1 is G in both orders, so swapping R and B in the input swaps planes 0 and 2 and nothing else"""
    P = 4096 + 33
    rgba = pixels(P, 4, 11).reshape(P, 4)
    bgra = rgba[:, [2, 1, 0, 3]]
    for decorrelate, layout in R.SETTINGS:
        a = R.forward(rgba.reshape(-1), 4, decorrelate, layout)
        b = R.forward(bgra.reshape(-1), 4, decorrelate, layout)
        if layout == R.INTERLEAVED:
            assert np.array_equal(a.reshape(P, 4)[:, [2, 1, 0, 3]], b.reshape(P, 4))
        else:
            assert np.array_equal(a.reshape(4, P)[[2, 1, 0, 3]], b.reshape(4, P))


# ---- the library, no device ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(pkg):
    return R.declare(C.CDLL(pkg._lib.lib_path()))


def test_header_words(lib):
    seen = set()
    for code in (R.TF_RGBA8888, R.TF_BGRA8888, R.TF_BGR888):
        for decorrelate, layout in R.SETTINGS:
            word = lib.dxtlt_transform_header_pack_pixels(code, decorrelate, layout)
            assert word == R.header_word(code, decorrelate, layout)
            assert word & 0xF == code and (word >> 4) & 3 == 0 and (word >> 16) == R.VENDOR_TAG
            seen.add(word)
            # upstream's unpack of its placeholder layout refuses the word: the reserved bits are not zero
            fmt, flag = C.c_int32(-1), C.c_bool(False)
            assert lib.dxtlt_transform_header_unpack_reserved_format(word, C.byref(fmt), C.byref(flag)) == FF_CORRUPTED
        assert lib.dxtlt_transform_header_pack_pixels(code, True, 3) == 0
    assert len(seen) == 18
    for code in (0, 1, 2, 3, 4, 8, 9, 15, -1):
        assert lib.dxtlt_transform_header_pack_pixels(code, True, 2) == 0


def test_arguments_are_checked_before_any_device_work(pkg, lib):
    import torch

    buf, out = np.zeros(96, dtype=np.uint8), np.zeros(96, dtype=np.uint8)
    p, q = buf.ctypes.data, out.ctypes.data
    for name in ("dxtlt_transform_pixels", "dxtlt_untransform_pixels", "dxtlt_transform_pixels_device", "dxtlt_untransform_pixels_device"):
        tail = (None,) if name.endswith("_device") else ()
        f = getattr(lib, name)
        assert f(p, q, 13, 4, True, 2, *tail) == E_LENGTH
        assert f(p, q, 16, 3, True, 2, *tail) == E_LENGTH
        assert f(p, q, 12, 5, True, 2, *tail) == E_ARGUMENT
        assert f(p, q, 12, 0, True, 2, *tail) == E_ARGUMENT
        assert f(p, q, 12, 4, True, 3, *tail) == E_ARGUMENT
        assert f(None, q, 12, 4, True, 2, *tail) == E_ARGUMENT
        assert f(p, None, 12, 3, True, 2, *tail) == E_ARGUMENT
        assert "dxtlt" in pkg._lib.last_error()
        assert f(None, None, 0, 4, True, 2, *tail) == OK          # nothing to do, no device needed
    r = lib.dxtlt_transform_pixels_range_device
    assert r(4, False, p, q, 5000, 100, 10, True, 2, None) == E_ARGUMENT      # first_pixel off a segment
    assert r(4, False, p, q, 5000, 4096, 905, True, 2, None) == E_ARGUMENT    # range outside total_pixels
    assert r(4, False, p, q, 5000, 8192, 0, True, 2, None) == E_ARGUMENT
    assert r(2, False, p, q, 24, 0, 24, True, 2, None) == E_ARGUMENT
    assert r(3, True, p, q, 24, 0, 24, True, 7, None) == E_ARGUMENT
    assert r(3, True, None, q, 24, 0, 24, True, 1, None) == E_ARGUMENT
    assert r(3, True, None, None, 24, 0, 0, True, 1, None) == OK
    # the generic sharded call with the pixel codes
    s = lib.dxtlt_transform_sharded
    assert s(8, False, p, q, 13, 1, True, True, 1) == E_LENGTH
    assert s(9, False, p, q, 13, 1, True, True, 1) == E_LENGTH
    assert s(9, False, None, q, 12, 1, True, True, 1) == E_ARGUMENT
    assert s(8, True, p, q, 0, 1, True, True, 1) == OK
    if not torch.cuda.is_available():
        # valid arguments reach the device path, and there is no CPU fallback behind it
        assert lib.dxtlt_transform_pixels(p, q, 96, 4, True, 2) == E_NO_DEVICE
        assert lib.dxtlt_untransform_pixels(p, q, 96, 3, False, 1) == E_NO_DEVICE
        assert lib.dxtlt_transform_pixels_device(p, q, 96, 4, True, 2, None) == E_NO_DEVICE
        assert lib.dxtlt_untransform_pixels_device(p, q, 96, 3, True, 0, None) == E_NO_DEVICE
        assert r(4, False, p, q, 24, 0, 24, True, 2, None) == E_NO_DEVICE
        assert s(8, False, p, q, 96, 1, True, True, 1) == E_NO_DEVICE
        assert "no HIP device" in pkg._lib.last_error()
        assert np.array_equal(out, np.zeros(96, dtype=np.uint8))


def test_host_batch_validates_pixel_items_with_the_rest(pkg, lib):
    from dxt_lossless_transform_amd.batch import DxtltBatchItem

    buf, out = np.zeros(96, dtype=np.uint8), np.zeros(96, dtype=np.uint8)
    p, q = buf.ctypes.data, out.ctypes.data

    def item(fmt, src, dst, n):
        it = DxtltBatchItem()
        it.d_input, it.d_output, it.len, it.format, it.decorrelation_mode, it.split_colour_endpoints = src, dst, n, fmt, 1, 1
        return it

    def call(f, *its, extra=()):
        arr = (DxtltBatchItem * len(its))(*its)
        return f(arr, len(its), *extra)

    host = lib.dxtlt_transform_batch_host
    host.argtypes, host.restype = [C.POINTER(DxtltBatchItem), C.c_size_t], C.c_int32
    assert call(host, item(1, p, q, 16), item(8, p, q, 13)) == E_LENGTH
    assert call(host, item(9, p, q, 16)) == E_LENGTH
    assert call(host, item(9, None, q, 12)) == E_ARGUMENT
    assert call(host, item(8, p, p + 4, 16)) == E_ARGUMENT          # input and output overlap
    assert call(host, item(10, p, q, 16)) == E_ARGUMENT
    assert "8 (4-byte pixels) or 9 (3-byte pixels" in pkg._lib.last_error()
    assert call(host, item(8, None, None, 0), item(9, None, None, 0)) == OK
    # the device batch call takes 1..7 as before: the pixel codes are refused there, whatever the item's length
    dev = lib.dxtlt_transform_batch_device
    dev.argtypes, dev.restype = [C.POINTER(DxtltBatchItem), C.c_size_t, C.c_void_p], C.c_int32
    for fmt, n in ((8, 16), (9, 12), (9, 64), (8, 0)):
        assert call(dev, item(fmt, p, q, n), extra=(None,)) == E_ARGUMENT
        assert "dxtlt_transform_batch_host" in pkg._lib.last_error()


# ---- DDS ---------------------------------------------------------------------------------------------------------------------
def dds_files():
    """(name, file bytes as an array, data offset, bytes per pixel, TransformFormat code)"""
    rng = np.random.default_rng(0xDD5)
    out = []
    for name, B, code, build in (("rgba-dx10", 4, R.TF_RGBA8888, lambda p: R.dds_dx10(p, 8, 4, 28)),
                                 ("bgra-dx10", 4, R.TF_BGRA8888, lambda p: R.dds_dx10(p, 8, 4, 87)),
                                 ("rgba-masks", 4, R.TF_RGBA8888, lambda p: R.dds_legacy(p, 8, 4, "rgba")),
                                 ("bgra-masks", 4, R.TF_BGRA8888, lambda p: R.dds_legacy(p, 8, 4, "bgra")),
                                 ("bgr-masks", 3, R.TF_BGR888, lambda p: R.dds_legacy(p, 8, 4, "bgr"))):
        f = np.frombuffer(build(rng.integers(0, 256, 32 * B, dtype=np.uint8).tobytes()) + b"end", dtype=np.uint8).copy()
        out.append((name, f, f.size - 3 - 32 * B, B, code))
    return out


@pytest.mark.parametrize("case", dds_files(), ids=lambda c: c[0])
def test_switch_off_refuses_pixel_payloads_and_codes(lib, case):
    _, f, off, B, code = case
    lib.dxtlt_file_formats_enable_pixels(False)
    out = np.full(f.size, 0xEE, dtype=np.uint8)
    est, calls = R.counting_estimator()
    assert lib.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, out.size, 1, True, True) == FF_UNKNOWN
    assert lib.dxtlt_dds_transform_auto(f.ctypes.data, f.size, out.ctypes.data, out.size, C.byref(est), False) == FF_UNKNOWN
    assert calls[0] == 0
    t = f.copy()
    struct.pack_into("<I", t, 0, R.header_word(code, True, R.PLANAR_DELTA))
    assert lib.dxtlt_dds_untransform(t.ctypes.data, t.size, out.ctypes.data, out.size) == FF_UNKNOWN
    for inverse, src in ((False, f), (True, t)):
        it = (R.DdsBatchItem * 1)()
        it[0].input, it[0].input_len, it[0].output, it[0].output_len, it[0].status = src.ctypes.data, src.size, out.ctypes.data, out.size, -1
        it[0].decorrelation_mode, it[0].split_alpha_endpoints, it[0].split_colour_endpoints = 1, True, True
        assert lib.dxtlt_dds_transform_batch(it, 1, inverse) == 1
        assert it[0].status == FF_UNKNOWN


@pytest.mark.parametrize("case", dds_files(), ids=lambda c: c[0])
def test_switch_on_checks_that_need_no_device(lib, case):
    _, f, off, B, code = case
    lib.dxtlt_file_formats_enable_pixels(True)
    try:
        out = np.zeros(f.size, dtype=np.uint8)
        # output too small
        assert lib.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, f.size - 1, 1, True, True) == FF_TOO_SMALL
        t = f.copy()
        struct.pack_into("<I", t, 0, R.header_word(code, True, R.PLANAR_DELTA))
        assert lib.dxtlt_dds_untransform(t.ctypes.data, t.size, out.ctypes.data, t.size - 1) == FF_TOO_SMALL
        # a word with the right code that is not one of the six: upstream's placeholder words, another version, layout 3, another tag
        good = R.header_word(code, True, R.PLANAR_DELTA)
        for word in (code, code | (1 << 6), good ^ (1 << 9), good | (3 << 7), good ^ (1 << 20), good | (1 << 4)):
            struct.pack_into("<I", t, 0, word)
            assert lib.dxtlt_dds_untransform(t.ctypes.data, t.size, out.ctypes.data, out.size) == FF_CORRUPTED, hex(word)
            it = (R.DdsBatchItem * 1)()
            it[0].input, it[0].input_len, it[0].output, it[0].output_len, it[0].status = t.ctypes.data, t.size, out.ctypes.data, out.size, -1
            assert lib.dxtlt_dds_transform_batch(it, 1, True) == 1 and it[0].status == FF_CORRUPTED
    finally:
        lib.dxtlt_file_formats_enable_pixels(False)


def test_switch_on_invalid_alignment(lib):
    """A payload length that is no multiple of the pixel size: a DDS length is a u32 whose products wrap and whose sum saturates
    (parse_dds), so 65535 x 65535 BGR (the product wraps to 4294574083 = 1 mod 3) and 65535 x 65535 RGBA with two levels (the sum
    saturates at 2^32 - 1 = 3 mod 4) state one.  The check precedes every access to the payload: the lengths passed are the
    stated ones, the memory behind the pointers is the header alone."""
    lib.parse_dds.argtypes, lib.parse_dds.restype = [C.c_void_p, C.c_size_t], C.c_uint64
    lib.dxtlt_file_formats_enable_pixels(True)
    try:
        for build, B, code, want in ((lambda: R.dds_legacy(b"", 65535, 65535, "bgr"), 3, R.TF_BGR888, 4294574083),
                                     (lambda: R.dds_dx10(b"", 65535, 65535, 28, 2), 4, R.TF_RGBA8888, 0xFFFFFFFF)):
            f = np.frombuffer(build(), dtype=np.uint8).copy()
            info = lib.parse_dds(f.ctypes.data, f.size)       # {u8 Format, u8 DataOffset, u32 DataLength} in one register
            assert info >> 32 == want and want % B != 0
            claimed = f.size + want
            out = np.zeros(f.size, dtype=np.uint8)
            assert lib.dxtlt_dds_transform(f.ctypes.data, claimed, out.ctypes.data, claimed, 1, True, True) == FF_ALIGNMENT
            est, calls = R.counting_estimator()
            assert lib.dxtlt_dds_transform_auto(f.ctypes.data, claimed, out.ctypes.data, claimed, C.byref(est), False) == FF_ALIGNMENT
            assert calls[0] == 0
            t = f.copy()
            struct.pack_into("<I", t, 0, R.header_word(code, True, R.PLANAR_DELTA))
            assert lib.dxtlt_dds_untransform(t.ctypes.data, claimed, out.ctypes.data, claimed) == FF_ALIGNMENT
            for inverse, src in ((False, f), (True, t)):
                it = (R.DdsBatchItem * 1)()
                it[0].input, it[0].input_len, it[0].output, it[0].output_len, it[0].status = src.ctypes.data, claimed, out.ctypes.data, claimed, -1
                assert lib.dxtlt_dds_transform_batch(it, 1, inverse) == 1 and it[0].status == FF_ALIGNMENT
            assert not out.any()
    finally:
        lib.dxtlt_file_formats_enable_pixels(False)
