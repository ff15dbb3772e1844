"""Uncompressed pixels on the MI355X: the kernels against the CPU statement (tests/pixels_ref.py), forward and
inverse-of-reference-forward, through the device, range, host, sharded, batch and DDS entry points.  Every device buffer sits
inside guard bytes that must be unchanged afterwards; every case is a few thousand pixels."""
import ctypes as C
import struct

import numpy as np
import pytest

import pixels_ref as R
from pixels_gpu_common import E_ARGUMENT, OK, Guarded, device_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return R.declare(C.CDLL(pkg._lib.lib_path()))


def pixels(P, B, seed):
    return np.random.default_rng(seed).integers(0, 256, P * B, dtype=np.uint8)


def check_both_directions(lib, dev, data, B, decorrelate, layout, in_off=0, out_off=0):
    want = R.forward(data, B, decorrelate, layout)
    got = device_call(lib, dev, False, data, B, decorrelate, layout, in_off, out_off)
    assert np.array_equal(got, want), ("forward", data.size // B, B, decorrelate, layout, in_off, out_off)
    back = device_call(lib, dev, True, want, B, decorrelate, layout, out_off, in_off)
    assert np.array_equal(back, data), ("inverse", data.size // B, B, decorrelate, layout, in_off, out_off)


SMALL = [0, 1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257]
EDGES = [4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 123]


@pytest.mark.parametrize("decorrelate,layout", R.SETTINGS)
@pytest.mark.parametrize("B", [3, 4])
def test_every_combination_at_small_counts(lib, dev, B, decorrelate, layout):
    """sub-vector heads and tails, planes shorter than one 16-byte store"""
    for P in SMALL:
        check_both_directions(lib, dev, pixels(P, B, 31 * P + B), B, decorrelate, layout)


@pytest.mark.parametrize("decorrelate,layout", R.SETTINGS)
@pytest.mark.parametrize("B", [3, 4])
def test_tile_and_segment_edges(lib, dev, B, decorrelate, layout):
    for P in EDGES:
        check_both_directions(lib, dev, pixels(P, B, P + B), B, decorrelate, layout)


@pytest.mark.parametrize("layout", [R.PLANAR, R.PLANAR_DELTA])
@pytest.mark.parametrize("B", [3, 4])
def test_every_plane_base_residue(lib, dev, B, layout):
    """16-byte aligned pointers: k = 0 is the fast form, k = 1..15 put plane c at residue c k mod 16"""
    for k in range(16):
        check_both_directions(lib, dev, pixels(4096 + k, B, 77 + k), B, True, layout)


@pytest.mark.parametrize("P", [4096 + 16, 8192 + 7])
@pytest.mark.parametrize("B", [3, 4])
def test_pointer_alignment(lib, dev, B, P):
    data = pixels(P, B, P * B)
    for in_off in (0, 1, 2, 3, 4, 8, 15):
        for out_off in (0, 1, 2, 3, 4, 8, 15):
            for decorrelate, layout in ((True, R.PLANAR_DELTA), (False, R.INTERLEAVED)):
                check_both_directions(lib, dev, data, B, decorrelate, layout, in_off, out_off)


def delta_planes():
    """named planes of deltas: what the prefix sum of the inverse has to carry across lanes, waves and segments"""
    P = 2 * 4096 + 300
    rng = np.random.default_rng(0x5CA)
    out = [("ones", np.ones(P, dtype=np.uint8)), ("255s", np.full(P, 255, dtype=np.uint8)),
           ("random", rng.integers(0, 256, P, dtype=np.uint8))]
    for pos in (0, 15, 16, 1023, 1024, 4095, 4096):
        d = np.zeros(P, dtype=np.uint8)
        d[pos] = 0x93
        out.append((f"single@{pos}", d))
    return out


@pytest.mark.parametrize("name,deltas", delta_planes(), ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("B", [3, 4])
def test_scan_carries(lib, dev, B, name, deltas):
    P = deltas.size
    other = pixels(P, 1, 5)
    # the deltas as PLANAR_DELTA input, in every plane in turn (random deltas elsewhere)
    for plane in range(B):
        planes = np.stack([deltas if c == plane else np.roll(other, c) for c in range(B)])
        for decorrelate in (False, True):
            got = device_call(lib, dev, True, planes.reshape(-1), B, decorrelate, R.PLANAR_DELTA)
            assert np.array_equal(got, R.inverse(planes.reshape(-1), B, decorrelate, R.PLANAR_DELTA)), (plane, decorrelate)
    # and forward of the matching ramps: the device's own deltas, and back
    ramp = np.concatenate([np.cumsum(deltas[s:s + 4096], dtype=np.uint8) for s in range(0, P, 4096)])
    px = np.stack([ramp] * B, axis=1).reshape(-1)
    fwd = device_call(lib, dev, False, px, B, False, R.PLANAR_DELTA)
    assert np.array_equal(fwd.reshape(B, P)[0], deltas)
    assert np.array_equal(device_call(lib, dev, True, fwd, B, False, R.PLANAR_DELTA), px)


@pytest.mark.parametrize("B", [3, 4])
def test_decorrelation_wraps_and_alpha_is_untouched(lib, dev, B):
    P = 4096 + 50
    alpha = pixels(P, 1, 9)
    for g, rb in ((255, 0), (0, 255)):
        px = np.zeros((P, B), dtype=np.uint8)
        px[:, 0], px[:, 1], px[:, 2] = rb, g, rb
        if B == 4:
            px[:, 3] = alpha
        for layout in R.LAYOUTS:
            got = device_call(lib, dev, False, px.reshape(-1), B, True, layout)
            assert np.array_equal(got, R.forward(px.reshape(-1), B, True, layout))
            if B == 4 and layout == R.PLANAR:
                assert np.array_equal(got.reshape(4, P)[3], alpha)
                assert (got.reshape(4, P)[0] == ((rb - g) & 0xFF)).all()
            assert np.array_equal(device_call(lib, dev, True, got, B, True, layout), px.reshape(-1))


@pytest.mark.parametrize("decorrelate,layout", [(True, R.PLANAR_DELTA), (False, R.PLANAR), (True, R.INTERLEAVED)])
@pytest.mark.parametrize("B", [3, 4])
def test_ranges_compose(lib, dev, B, decorrelate, layout):
    import torch

    P = 5 * 4096 + 77
    data = pixels(P, B, 123 + B)
    whole = R.forward(data, B, decorrelate, layout)
    assert np.array_equal(device_call(lib, dev, False, data, B, decorrelate, layout), whole)
    cuts = [(4096, 3 * 4096), (3 * 4096, P), (0, 4096)]      # shuffled order
    stream = torch.cuda.current_stream().cuda_stream
    r = lib.dxtlt_transform_pixels_range_device
    src, dst = Guarded(dev, data.size, 0, data), Guarded(dev, data.size)
    for a, b in cuts:
        assert r(B, False, src.ptr + a * B, dst.ptr, P, a, b - a, decorrelate, layout, stream) == OK
    torch.cuda.synchronize()
    assert np.array_equal(dst.bytes(), whole)
    back = Guarded(dev, data.size)
    for a, b in cuts:
        assert r(B, True, dst.ptr, back.ptr + a * B, P, a, b - a, decorrelate, layout, stream) == OK
    torch.cuda.synchronize()
    assert np.array_equal(back.bytes(), data)
    # a first_pixel off a segment: refused, nothing written
    fresh = Guarded(dev, data.size)
    assert r(B, False, src.ptr + 100 * B, fresh.ptr, P, 100, 4096, decorrelate, layout, stream) == E_ARGUMENT
    torch.cuda.synchronize()
    assert (fresh.bytes() == 0xA5).all()


@pytest.mark.parametrize("P", [12_411, 400_003])
@pytest.mark.parametrize("B", [3, 4])
def test_host_buffers(lib, B, P):
    """12 411 pixels: mapped staging; 400 003: above the mapped limit (1 MiB), below the pipeline threshold (96 MiB)"""
    data = pixels(P, B, P)
    for decorrelate, layout in R.SETTINGS:
        out, back = np.zeros_like(data), np.zeros_like(data)
        assert lib.dxtlt_transform_pixels(data.ctypes.data, out.ctypes.data, data.size, B, decorrelate, layout) == OK
        assert np.array_equal(out, R.forward(data, B, decorrelate, layout))
        assert lib.dxtlt_untransform_pixels(out.ctypes.data, back.ctypes.data, data.size, B, decorrelate, layout) == OK
        assert np.array_equal(back, data)


@pytest.mark.parametrize("code,B", [(8, 4), (9, 3)])
def test_sharded_equals_reference(lib, code, B):
    P = 3 * 4096 + 123
    data = pixels(P, B, 55 + B)
    for decorrelate, layout in R.SETTINGS:
        mode, sa, sc = R.triple_of(decorrelate, layout)
        out, back = np.zeros_like(data), np.zeros_like(data)
        assert lib.dxtlt_transform_sharded(code, False, data.ctypes.data, out.ctypes.data, data.size, mode, sa, sc, 3) == OK
        assert np.array_equal(out, R.forward(data, B, decorrelate, layout)), (decorrelate, layout)
        assert lib.dxtlt_transform_sharded(code, True, out.ctypes.data, back.ctypes.data, data.size, mode, sa, sc, 3) == OK
        assert np.array_equal(back, data)


def test_mixed_host_batch_equals_single_calls(pkg, lib, dev):
    """One dxtlt_transform_batch_host call mixing BC1 items with code-8 and code-9 items of different settings: each item
    equals its single-buffer result.  (The device batch call does not take the pixel codes: tests/test_pixels.py.)"""
    import torch

    from dxt_lossless_transform_amd import batch

    rng = np.random.default_rng(0xBA7)
    plan = [("bc1", False, rng.integers(0, 256, 8 * 3000, dtype=np.uint8), pkg.Bc1TransformSettings()),
            ("pixels4", False, pixels(5 * 4096 + 77, 4, 1), (True, R.PLANAR_DELTA)),
            ("bc1", True, rng.integers(0, 256, 8 * 1025, dtype=np.uint8), pkg.Bc1TransformSettings()),
            ("pixels3", False, pixels(4096 + 33, 3, 2), (False, R.PLANAR)),
            ("pixels3", True, pixels(87_381, 3, 3), (True, R.PLANAR_DELTA)),
            ("pixels4", True, pixels(257, 4, 4), (True, R.INTERLEAVED))]
    want = []
    for fmt, inverse, host, st in plan:
        if fmt == "bc1":
            x = torch.from_numpy(host).to(dev)
            ref = torch.zeros_like(x)
            getattr(pkg, f"{'untransform' if inverse else 'transform'}_bc1_with_settings")(x, ref, st)
            want.append(ref.cpu().numpy())
        else:
            B = 4 if fmt == "pixels4" else 3
            single = device_call(lib, dev, inverse, host, B, *st)
            assert np.array_equal(single, (R.inverse if inverse else R.forward)(host, B, *st))
            want.append(single)
    # odd host addresses for the pixel items, guard bytes around every output
    ins, outs = [], []
    for k, (fmt, _, h, _) in enumerate(plan):
        off = 0 if fmt == "bc1" else 1 + 2 * k
        i = np.zeros(h.size + 64, dtype=np.uint8)
        i[off:off + h.size] = h
        ins.append(i[off:off + h.size])
        o = np.full(h.size + 64, 0xA5, dtype=np.uint8)
        outs.append((o, off + 3))
    batch.transform_batch_host([(fmt, inverse, i, o[at:at + i.size], st) for (fmt, inverse, _, st), i, (o, at) in zip(plan, ins, outs)])
    for (o, at), ref, (fmt, inverse, host, _) in zip(outs, want, plan):
        assert np.array_equal(o[at:at + host.size], ref), (fmt, inverse, host.size)
        assert (o[:at] == 0xA5).all() and (o[at + host.size:] == 0xA5).all()


# ---- DDS -----------------------------------------------------------------------------------------------------------------------
def dds_cases():
    """(name, file, data offset, bytes per pixel, TransformFormat code): 64 x 64 with and without its 7-level chain (5 461 pixels)"""
    out = []
    for mips in (1, 7):
        n = R.mip_pixels(64, 64, mips)
        for name, B, code, build in (("rgba-dx10", 4, R.TF_RGBA8888, lambda p, m: R.dds_dx10(p, 64, 64, 28, m)),
                                     ("bgra-dx10", 4, R.TF_BGRA8888, lambda p, m: R.dds_dx10(p, 64, 64, 87, m)),
                                     ("rgba-masks", 4, R.TF_RGBA8888, lambda p, m: R.dds_legacy(p, 64, 64, "rgba", m)),
                                     ("bgr-masks", 3, R.TF_BGR888, lambda p, m: R.dds_legacy(p, 64, 64, "bgr", m))):
            payload = pixels(n, B, 17 * mips + B + len(name)).tobytes()
            f = np.frombuffer(build(payload, mips) + b"end", dtype=np.uint8).copy()
            out.append((f"{name}-{mips}", f, f.size - 3 - n * B, B, code))
    return out


@pytest.fixture
def pixels_on(lib):
    lib.dxtlt_file_formats_enable_pixels(True)
    try:
        yield lib
    finally:
        lib.dxtlt_file_formats_enable_pixels(False)


@pytest.mark.parametrize("case", dds_cases(), ids=lambda c: c[0])
def test_dds_round_trip(pixels_on, case):
    lib = pixels_on
    _, f, off, B, code = case
    end = f.size - 3
    for decorrelate, layout in R.SETTINGS:
        mode, sa, sc = R.triple_of(decorrelate, layout)
        out = np.zeros_like(f)
        assert lib.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, out.size, mode, sa, sc) == 0
        word = struct.unpack_from("<I", out.tobytes())[0]
        assert word == lib.dxtlt_transform_header_pack_pixels(code, decorrelate, layout) == R.header_word(code, decorrelate, layout)
        assert np.array_equal(out[off:end], R.forward(f[off:end], B, decorrelate, layout))
        assert out[4:off].tobytes() == f[4:off].tobytes() and out[end:].tobytes() == b"end"
        back = np.zeros_like(f)
        assert lib.dxtlt_dds_untransform(out.ctypes.data, out.size, back.ctypes.data, back.size) == 0
        assert back.tobytes() == f.tobytes()


def test_dds_auto_is_the_fixed_setting_without_estimation(pixels_on):
    lib = pixels_on
    u64 = C.c_uint64
    lib.dxtlt_debug_auto_last_estimation.argtypes, lib.dxtlt_debug_auto_last_estimation.restype = [C.POINTER(u64), C.POINTER(u64)], None
    before = (u64(), u64())
    lib.dxtlt_debug_auto_last_estimation(C.byref(before[0]), C.byref(before[1]))
    for _, f, off, B, code in dds_cases():
        est, calls = R.counting_estimator()
        out = np.zeros_like(f)
        assert lib.dxtlt_dds_transform_auto(f.ctypes.data, f.size, out.ctypes.data, out.size, C.byref(est), True) == 0
        assert calls[0] == 0
        assert struct.unpack_from("<I", out.tobytes())[0] == R.header_word(code, True, R.PLANAR_DELTA)
        assert np.array_equal(out[off:f.size - 3], R.forward(f[off:f.size - 3], B, True, R.PLANAR_DELTA))
        back = np.zeros_like(f)
        assert lib.dxtlt_dds_untransform(out.ctypes.data, out.size, back.ctypes.data, back.size) == 0
        assert back.tobytes() == f.tobytes()
    after = (u64(), u64())
    lib.dxtlt_debug_auto_last_estimation(C.byref(after[0]), C.byref(after[1]))
    assert (after[0].value, after[1].value) in ((before[0].value, before[1].value), (0, 0))


def test_dds_batch_mixes_formats_and_reports_the_corrupt_file(pixels_on):
    lib = pixels_on
    cases = {c[0]: c for c in dds_cases()}
    bc1 = np.frombuffer(R.dds_dx10(pixels(8 * 300, 1, 5).tobytes(), 80, 60, 71) + b"end", dtype=np.uint8).copy()
    corrupt = cases["rgba-masks-1"][1][:100].copy()                 # shorter than a DDS header
    files = [bc1, cases["rgba-dx10-7"][1], cases["bgr-masks-7"][1], corrupt]
    mode, sa, sc = R.triple_of(True, R.PLANAR_DELTA)
    singles, single_status = [], []
    for f in files:
        o = np.zeros_like(f)
        single_status.append(lib.dxtlt_dds_transform(f.ctypes.data, f.size, o.ctypes.data, o.size, mode, sa, sc))
        singles.append(o)
    assert single_status[:3] == [0, 0, 0] and single_status[3] != 0
    items = (R.DdsBatchItem * len(files))()
    outs = [np.zeros_like(f) for f in files]
    for it, f, o in zip(items, files, outs):
        it.input, it.input_len, it.output, it.output_len, it.status = f.ctypes.data, f.size, o.ctypes.data, o.size, -1
        it.decorrelation_mode, it.split_alpha_endpoints, it.split_colour_endpoints = mode, sa, sc
    assert lib.dxtlt_dds_transform_batch(items, len(files), False) == 1
    assert [it.status for it in items] == single_status
    for o, s in list(zip(outs, singles))[:3]:
        assert o.tobytes() == s.tobytes()
    # inverse: the three transformed files and one whose word is not one of the six
    bad = outs[1].copy()
    struct.pack_into("<I", bad, 0, struct.unpack_from("<I", bad.tobytes())[0] ^ (1 << 9))
    sources = outs[:3] + [bad]
    backs = [np.zeros_like(s) for s in sources]
    want_status = []
    for s in sources:
        b = np.zeros_like(s)
        want_status.append(lib.dxtlt_dds_untransform(s.ctypes.data, s.size, b.ctypes.data, b.size))
    assert want_status == [0, 0, 0, 5]
    for it, s, b in zip(items, sources, backs):
        it.input, it.input_len, it.output, it.output_len, it.status = s.ctypes.data, s.size, b.ctypes.data, b.size, -1
    assert lib.dxtlt_dds_transform_batch(items, len(sources), True) == 1
    assert [it.status for it in items] == want_status
    for b, f in list(zip(backs, files))[:3]:
        assert b.tobytes() == f.tobytes()
