"""The entropy estimator, version 1 (docs/ESTIMATOR.md), without a device: the table the library carries against the definition,
the CPU statement's closed forms, the quality of the pixel auto transform's pick with it, and the argument checks of the new
calls (which run before any device work)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import entropy_ref as R
import pixels_auto_data as D
import pixels_ref


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, sz, i32, u64p = C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_uint64)
    l.dxtlt_entropy_estimator_version.restype = C.c_uint32
    l.dxtlt_debug_entropy_table.argtypes, l.dxtlt_debug_entropy_table.restype = [C.c_uint32], C.c_uint32
    l.dxtlt_estimate_entropy_sizes_device.argtypes, l.dxtlt_estimate_entropy_sizes_device.restype = [vp, sz, vp, vp], i32
    l.dxtlt_estimate_entropy_size_device.argtypes, l.dxtlt_estimate_entropy_size_device.restype = [vp, sz, vp, u64p], i32
    l.dxtlt_estimate_entropy_size.argtypes, l.dxtlt_estimate_entropy_size.restype = [vp, sz, u64p], i32
    l.dxtlt_builtin_entropy_estimator.restype = C.POINTER(pixels_ref.Estimator)
    l.dxtlt_transform_pixels_auto.argtypes = [vp, vp, sz, i32, C.POINTER(pixels_ref.Estimator), C.POINTER(C.c_bool), C.POINTER(C.c_uint8)]
    l.dxtlt_transform_pixels_auto.restype = i32
    l.dxtlt_transform_pixels_auto_device.argtypes = [vp, vp, sz, i32, vp, C.POINTER(C.c_bool), C.POINTER(C.c_uint8)]
    l.dxtlt_transform_pixels_auto_device.restype = i32
    l.dxtlt_debug_pixels_auto_last_totals.argtypes, l.dxtlt_debug_pixels_auto_last_totals.restype = [u64p, i32], i32
    l.dxtlt_debug_auto_last_estimation.argtypes, l.dxtlt_debug_auto_last_estimation.restype = [u64p, u64p], None
    l.dxtlt_file_formats_enable_pixel_auto.argtypes, l.dxtlt_file_formats_enable_pixel_auto.restype = [C.c_bool], None
    return l


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_reference_table_anchors_and_worked_vector():
    assert R.T[0] == 0 and R.T[1] == 0
    for k, v in R.ANCHORS.items():
        assert R.T[k] == v, k
    b = np.frombuffer(R.WORKED_VECTOR, dtype=np.uint8)
    assert R.window_cost(b) == R.WORKED_COST == 16 * 262144 - (4 * 3 * 103872 + 4 * 131072)
    assert R.estimate(b) == R.WORKED_ESTIMATE


def test_library_table_is_the_definition_at_every_k(lib):
    assert lib.dxtlt_entropy_estimator_version() == R.VERSION
    got = np.array([lib.dxtlt_debug_entropy_table(k) for k in range(R.W + 1)], dtype=np.int64)
    assert np.array_equal(got, R.T)
    assert lib.dxtlt_debug_entropy_table(R.W + 1) == 0


def test_committed_table_header_is_what_its_generator_writes():
    from tools import gen_entropy_table

    assert open(gen_entropy_table.PATH).read() == gen_entropy_table.render()
    assert np.array_equal(np.array(gen_entropy_table.table(), dtype=np.int64), R.T)


# ---- closed forms of the statement ------------------------------------------------------------------------------------------------
def test_closed_forms():
    assert R.estimate(np.full(R.W, 0xFF, dtype=np.uint8)) == 0                      # a constant window
    assert R.estimate(np.full(3 * R.W + 5, 7, dtype=np.uint8)) == 0
    flat = np.repeat(np.arange(256, dtype=np.uint8), 128)                          # every value 128 times: 8 bits a byte
    assert flat.size == R.W and R.estimate(flat) == R.W
    rng = np.random.default_rng(0xE27)
    x = rng.integers(0, 40, R.W, dtype=np.uint8)
    assert R.estimate(rng.permutation(x)) == R.estimate(x)                          # order inside a window does not count
    assert R.estimate(np.zeros(0, dtype=np.uint8)) == 0 and R.estimate(None) == 0   # an empty section
    # split n - 1 / 1: log2 n + (n - 1) log2(n / (n - 1)) = 15 + 1.4427 bits, and each floor moves q by less than one unit per
    # byte counted (n units, half a bit): between 16 and 17 bits, three bytes rounded up
    two = np.zeros(R.W, dtype=np.uint8)
    two[123] = 1
    assert 16 << 16 < R.section_cost(two) < 17 << 16 and R.estimate(two) == 3
    # windows are counted from the section's first byte, the last one shorter, and rounded up once per section
    y = rng.integers(0, 256, 2 * R.W + 777, dtype=np.uint8)
    parts = [R.window_cost(y[:R.W]), R.window_cost(y[R.W:2 * R.W]), R.window_cost(y[2 * R.W:])]
    assert R.estimate(y) == (sum(parts) + (1 << 19) - 1) >> 19


# ---- quality of the pick --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(7))
def test_entropy_pick_is_the_zlib_minimum(k):
    """On every data set the candidate the entropy statement picks, in candidate order with strict `<`, is the one zlib-6 makes
    smallest -- 1, 1, 1, 4, 4, 4, 4 in the 1-based order.  A condition on the inputs: if one stops satisfying it, change the input."""
    name, px, want = D.data_sets()[k]
    B, flat = px.shape[1], px.reshape(-1)
    totals, at, _ = R.auto(flat, B)
    z = [len(zlib.compress(pixels_ref.forward(flat, B, d, l).tobytes(), 6)) for d, l in R.CANDIDATES]
    print(name, "entropy", totals, "zlib-6", z)
    assert at + 1 == want, (name, totals)
    assert int(np.argmin(z)) + 1 == want and sorted(z)[0] < sorted(z)[1], (name, z)


def test_pick_rule():
    assert R.pick([5, 5, 5, 5, 5, 5]) == 0 and R.pick([0] * 6) == 0            # ties keep the first
    assert R.pick([9, 8, 8, 7, 7, 9]) == 3
    assert R.pick([(1 << 64) - 1] * 6) == 0
    assert R.CANDIDATES[0] == (True, pixels_ref.PLANAR_DELTA) and R.CANDIDATES[5] == (False, pixels_ref.INTERLEAVED)


# ---- argument checks, before any device work ---------------------------------------------------------------------------------------
def test_estimator_calls_validate_without_a_device(lib):
    out = C.c_uint64(99)
    assert lib.dxtlt_estimate_entropy_sizes_device(None, 0, None, None) == 0
    assert lib.dxtlt_estimate_entropy_sizes_device(None, 3, None, None) == 2
    sec = (C.c_uint64 * 2)(0, 0)
    assert lib.dxtlt_estimate_entropy_sizes_device(C.addressof(sec), 1, None, 12) == 2      # d_out off an 8-byte boundary
    assert lib.dxtlt_estimate_entropy_size_device(None, 10, None, None) == 2
    assert lib.dxtlt_estimate_entropy_size_device(None, 10, None, C.byref(out)) == 0 and out.value == 0   # NULL estimates as 0
    out.value = 99
    buf = np.zeros(16, dtype=np.uint8)
    assert lib.dxtlt_estimate_entropy_size(buf.ctypes.data, 0, C.byref(out)) == 0 and out.value == 0     # so does L == 0
    assert lib.dxtlt_estimate_entropy_size(buf.ctypes.data, 16, None) == 2
    e = lib.dxtlt_builtin_entropy_estimator()
    assert e and not e.contents.Context
    size = C.c_size_t(5)
    assert e.contents.MaxCompressedSize(None, 1000, C.byref(size)) == 0 and size.value == 0
    assert C.addressof(lib.dxtlt_builtin_entropy_estimator().contents) == C.addressof(e.contents)


def test_pixel_auto_calls_validate_without_a_device(lib):
    x, y = np.zeros(48, dtype=np.uint8), np.zeros(48, dtype=np.uint8)
    est = lib.dxtlt_builtin_entropy_estimator()
    dec, lay = C.c_bool(False), C.c_uint8(9)
    p, q = x.ctypes.data, y.ctypes.data
    for B in (0, 1, 2, 5):
        assert lib.dxtlt_transform_pixels_auto(p, q, 48, B, est, None, None) == 2
        assert lib.dxtlt_transform_pixels_auto_device(p, q, 48, B, None, None, None) == 2
    assert lib.dxtlt_transform_pixels_auto(p, q, 47, 4, est, None, None) == 1          # INVALID_LENGTH
    assert lib.dxtlt_transform_pixels_auto(p, q, 47, 3, est, None, None) == 1
    assert lib.dxtlt_transform_pixels_auto_device(p, q, 46, 4, None, None, None) == 1
    assert lib.dxtlt_transform_pixels_auto(p, q, 47, 7, est, None, None) == 2          # pixel_bytes is checked first
    assert lib.dxtlt_transform_pixels_auto(p, q, 48, 4, None, None, None) == 2         # NULL estimator, as the BC4 auto
    assert lib.dxtlt_transform_pixels_auto(p, q, 47, 4, None, None, None) == 1         # ... after the length
    assert lib.dxtlt_transform_pixels_auto(None, q, 48, 4, est, None, None) == 2
    assert lib.dxtlt_transform_pixels_auto(p, None, 48, 4, est, None, None) == 2
    assert lib.dxtlt_transform_pixels_auto_device(None, q, 48, 4, None, None, None) == 2
    assert lib.dxtlt_transform_pixels_auto_device(p, None, 48, 3, None, None, None) == 2
    # an empty buffer needs no device and keeps the first candidate; nothing is estimated
    for B in (3, 4):
        dec.value, lay.value = False, 9
        assert lib.dxtlt_transform_pixels_auto(None, None, 0, B, est, C.byref(dec), C.byref(lay)) == 0
        assert (dec.value, lay.value) == (True, 2)
        dec.value, lay.value = False, 9
        assert lib.dxtlt_transform_pixels_auto_device(None, None, 0, B, None, C.byref(dec), C.byref(lay)) == 0
        assert (dec.value, lay.value) == (True, 2)
        assert lib.dxtlt_debug_pixels_auto_last_totals(None, 0) == 0
    counting, calls = pixels_ref.counting_estimator()
    assert lib.dxtlt_transform_pixels_auto(None, None, 0, 4, C.byref(counting), C.byref(dec), C.byref(lay)) == 0 and calls[0] == 0
    a, b = C.c_uint64(7), C.c_uint64(7)
    lib.dxtlt_debug_auto_last_estimation(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    lib.dxtlt_file_formats_enable_pixel_auto(False)      # the switch exists and is off by default


def test_python_layer_exposes_the_new_calls(pkg):
    from dxt_lossless_transform_amd import estimator, pixels

    assert estimator.entropy_version() == R.VERSION
    assert estimator.entropy_table(3) == 103872
    assert estimator.estimate_entropy_size(b"") == 0
    assert estimator.builtin_entropy_estimator()
    assert pixels.AUTO_CANDIDATES == [(d, l) for d, l in R.CANDIDATES]
    out = np.zeros(0, dtype=np.uint8)
    assert pixels.transform_auto(np.zeros(0, dtype=np.uint8), out, 3) == (True, pixels.PLANAR_DELTA)
    with pytest.raises(pkg.InvalidLength):
        pixels.transform_auto(np.zeros(7, dtype=np.uint8), np.zeros(7, dtype=np.uint8), 4)
