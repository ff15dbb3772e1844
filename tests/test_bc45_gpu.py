"""BC4 / BC5 on the MI355X: every tile form (aligned, halo / shifted, edge) against the CPU restatement (tests/bc45_ref.py) and by
round trip, through the host, device, range, batch, DDS and auto entry points."""
import ctypes as C
import struct

import numpy as np
import pytest

import bc45_ref
import cabi

pytestmark = pytest.mark.gpu

FORMATS = ("bc4", "bc5")
COUNTS = [1, 2, 3, 127, 128, 129, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, 1_000_003]


def settings_of(pkg, fmt, split):
    return (pkg.Bc4TransformSettings if fmt == "bc4" else pkg.Bc5TransformSettings)(split)


def data(fmt, n, seed):
    return np.random.default_rng(seed).integers(0, 256, n * bc45_ref.BLOCK[fmt], dtype=np.uint8)


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n", COUNTS)
def test_device_buffers_match_reference(pkg, dev, fmt, split, n):
    import torch

    host = data(fmt, n, n * 7 + (fmt == "bc5") + 2 * split)
    want = bc45_ref.transform(fmt, host, split)
    st = settings_of(pkg, fmt, split)
    x = torch.from_numpy(host).to(dev)
    y, z = torch.empty_like(x), torch.empty_like(x)
    getattr(pkg, f"transform_{fmt}_with_settings")(x, y, st)
    getattr(pkg, f"untransform_{fmt}_with_settings")(y, z, st)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), want)
    assert torch.equal(z, x)


# Blocks per tile = tile_blocks(fmt, lanes) = lanes * 16 / block bytes (csrc/bcn_device.h).  BC5 launches every tile form with 256
# lanes: 256 blocks.  BC4 launches its aligned tiles with 128 lanes (default_tile_threads: 256 blocks) and its halo, shifted and edge
# tiles with 256 (shift_tile_threads / halo_tile_threads, plan_launches in csrc/bcn_kernels.hip: 512 blocks); the batch launch takes
# 256 lanes for all of them (batch_tile_threads).  The table holds the larger figure, so "four tiles" covers four of either.
TILE = {"bc4": 512, "bc5": 256}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("split", [False, True])
def test_every_n_through_four_tiles(pkg, dev, fmt, split):
    """Every block count from 1 through four tiles + 17 (every alignment class of the stream bases, every fill of the edge tile):
    forward == bc45_ref.transform, inverse of that == input.  All counts through the batch call, a few hundred buffers per
    call in one arena with 64 guard bytes behind each, and a seeded sample of 200 counts through the single-buffer call; then
    the sample once more with halo / shifted tiles forced."""
    import torch

    from dxt_lossless_transform_amd import batch

    B = bc45_ref.BLOCK[fmt]
    st = settings_of(pkg, fmt, split)
    top = 4 * TILE[fmt] + 17
    counts = list(range(1, top + 1))
    pool = data(fmt, top + 64, 0xE4E7 + (fmt == "bc5") + 2 * split)
    xs = {n: pool[(n % 64) * B:(n % 64 + n) * B] for n in counts}      # no two neighbours start alike
    wants = {n: bc45_ref.transform(fmt, xs[n], split) for n in counts}
    sample = sorted(np.random.default_rng(0x5A4D + len(fmt) + split).choice(counts, size=200, replace=False).tolist())
    guard = 64

    def through_the_batch_call(tag):
        for lo in range(0, len(counts), 300):
            chunk = counts[lo:lo + 300]
            offs, at = [], guard
            for n in chunk:
                offs.append(at)
                at += n * B + guard
            for inverse, srcs, expect, fill in ((False, xs, wants, 0xA5), (True, wants, xs, 0x5A)):
                h = np.zeros(at, dtype=np.uint8)
                for n, o in zip(chunk, offs):
                    h[o:o + n * B] = srcs[n]
                src = torch.from_numpy(h).to(dev)
                dst = torch.full((at,), fill, dtype=torch.uint8, device=dev)
                batch.transform_batch([(fmt, inverse, src[o:o + n * B], dst[o:o + n * B], st) for n, o in zip(chunk, offs)])
                torch.cuda.synchronize()
                got = dst.cpu().numpy()
                assert (got[:guard] == fill).all(), (tag, inverse, chunk[0])
                for n, o in zip(chunk, offs):
                    assert np.array_equal(got[o:o + n * B], expect[n]), (tag, "batch", inverse, n)
                    assert (got[o + n * B:o + n * B + guard] == fill).all(), (tag, "batch wrote outside", inverse, n)

    def through_the_single_call(tag):
        for n in sample:
            dst = torch.full((n * B + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
            back = torch.full((n * B + 2 * guard,), 0x5A, dtype=torch.uint8, device=dev)
            getattr(pkg, f"transform_{fmt}_with_settings")(torch.from_numpy(xs[n]).to(dev), dst[guard:guard + n * B], st)
            getattr(pkg, f"untransform_{fmt}_with_settings")(torch.from_numpy(wants[n]).to(dev), back[guard:guard + n * B], st)
            torch.cuda.synchronize()
            got, rt = dst.cpu().numpy(), back.cpu().numpy()
            assert np.array_equal(got[guard:guard + n * B], wants[n]), (tag, "forward", n)
            assert (got[:guard] == 0xA5).all() and (got[guard + n * B:] == 0xA5).all(), (tag, "forward wrote outside", n)
            assert np.array_equal(rt[guard:guard + n * B], xs[n]), (tag, "inverse", n)
            assert (rt[:guard] == 0x5A).all() and (rt[guard + n * B:] == 0x5A).all(), (tag, "inverse wrote outside", n)

    through_the_batch_call("default")
    through_the_single_call("default")
    try:
        pkg.set_tuning(0, 2)          # halo / shifted tiles always (the batch call plans per buffer and does not read the lever)
        through_the_single_call("forced")
    finally:
        pkg.set_tuning(0, 0)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n", [1, 129, (1 << 16) + 1, 1_000_003])
def test_host_buffers_match_reference(pkg, fmt, split, n):
    host = data(fmt, n, 31 * n + split)
    st = settings_of(pkg, fmt, split)
    y, z = np.zeros_like(host), np.zeros_like(host)
    getattr(pkg, f"transform_{fmt}_with_settings")(host, y, st)
    getattr(pkg, f"untransform_{fmt}_with_settings")(y, z, st)
    assert np.array_equal(y, bc45_ref.transform(fmt, host, split))
    assert np.array_equal(z, host)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n", [3, 4096, 70_001])
def test_pointer_offsets(pkg, dev, fmt, split, n):
    """Both buffers at byte offsets 1..15 from a 256-byte aligned allocation: unaligned AoS accesses and every stream shift"""
    import torch

    B = bc45_ref.BLOCK[fmt]
    host = data(fmt, n, 5 * n + split)
    want = bc45_ref.transform(fmt, host, split)
    st = settings_of(pkg, fmt, split)
    base_in = torch.zeros(n * B + 64, dtype=torch.uint8, device=dev)
    base_out = torch.zeros(n * B + 64, dtype=torch.uint8, device=dev)
    base_back = torch.zeros(n * B + 64, dtype=torch.uint8, device=dev)
    for off in range(1, 16):
        oo = (off * 7) % 16
        x = base_in[off:off + n * B]
        x.copy_(torch.from_numpy(host).to(dev))
        base_out.fill_(0xA5)
        y = base_out[oo:oo + n * B]
        z = base_back[off:off + n * B]
        getattr(pkg, f"transform_{fmt}_with_settings")(x, y, st)
        getattr(pkg, f"untransform_{fmt}_with_settings")(y, z, st)
        torch.cuda.synchronize()
        out = base_out.cpu().numpy()
        assert np.array_equal(out[oo:oo + n * B], want), (off, oo)
        assert (out[:oo] == 0xA5).all() and (out[oo + n * B:] == 0xA5).all(), (off, oo)   # nothing outside the buffer
        assert torch.equal(z, x), (off, oo)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("split", [False, True])
def test_ranges_stitch_to_the_whole_call(pkg, dev, fmt, split):
    import torch

    B = bc45_ref.BLOCK[fmt]
    n = 300_007
    host = data(fmt, n, 99 + split)
    st = settings_of(pkg, fmt, split)
    x = torch.from_numpy(host).to(dev)
    whole = torch.empty_like(x)
    getattr(pkg, f"transform_{fmt}_with_settings")(x, whole, st)
    cuts = [0, 1, 255, 4096, 77_777, 200_000, n]
    soa = torch.zeros_like(x)
    for a, b in zip(cuts, cuts[1:]):
        pkg.transform_range(fmt, False, x[a * B:b * B], soa, n, a, b - a, st)
    back = torch.zeros_like(x)
    for a, b in zip(cuts, cuts[1:]):
        pkg.transform_range(fmt, True, soa, back[a * B:b * B], n, a, b - a, st)
    torch.cuda.synchronize()
    assert torch.equal(soa, whole)
    assert torch.equal(back, x)


def test_mixed_batch_equals_one_call_per_item(pkg, dev, oracle):
    import torch

    from dxt_lossless_transform_amd import batch, bc7

    rng = np.random.default_rng(0xBA45)
    plan = []
    for k in range(30):
        fmt = ("bc1", "bc3", "bc4", "bc5", "bc7")[k % 5]
        n = int(rng.choice([1, 3, 129, 4096, 65_537, int(rng.integers(1, 200_000))]))
        inverse = bool(k % 3 == 2) and fmt != "bc7"
        if fmt == "bc1":
            st = pkg.Bc1TransformSettings(pkg.YCoCgVariant(int(rng.integers(0, 4))), bool(rng.integers(0, 2)))
        elif fmt == "bc3":
            st = pkg.Bc3TransformSettings(pkg.YCoCgVariant(int(rng.integers(0, 4))), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
        elif fmt == "bc7":
            st = None
        else:
            st = settings_of(pkg, fmt, bool(rng.integers(0, 2)))
        B = 16 if fmt == "bc7" else pkg.BLOCK_BYTES[fmt]
        host = rng.integers(0, 256, n * B, dtype=np.uint8)
        if fmt == "bc7":
            oracle.bc7_force_modes(host)
        plan.append((fmt, inverse, host, st))
    items, outs, want = [], [], []
    for fmt, inverse, host, st in plan:
        x = torch.from_numpy(host).to(dev)
        y = torch.zeros_like(x)
        ref = torch.zeros_like(x)
        if fmt == "bc7":
            (bc7.untransform_bc7 if inverse else bc7.transform_bc7)(x, ref)
        else:
            getattr(pkg, f"{'untransform' if inverse else 'transform'}_{fmt}_with_settings")(x, ref, st)
        items.append((fmt, inverse, x, y, st))
        outs.append(y)
        want.append(ref)
    batch.transform_batch(items)
    torch.cuda.synchronize()
    for (fmt, inverse, host, st), y, ref in zip(plan, outs, want):
        assert torch.equal(y, ref), (fmt, inverse, host.size)
        if fmt in ("bc4", "bc5"):
            f = bc45_ref.untransform if inverse else bc45_ref.transform
            assert np.array_equal(y.cpu().numpy(), f(fmt, host, st.split_endpoints))
    # the host batch: the same items as host buffers
    host_items, host_outs = [], []
    for fmt, inverse, host, st in plan:
        o = np.zeros_like(host)
        host_items.append((fmt, inverse, host, o, st))
        host_outs.append(o)
    batch.transform_batch_host(host_items)
    for o, ref in zip(host_outs, want):
        assert np.array_equal(o, ref.cpu().numpy())


# ---- DDS ---------------------------------------------------------------------------------------------------------
class DdsBatchItem(C.Structure):
    _fields_ = [("input", C.c_void_p), ("input_len", C.c_size_t), ("output", C.c_void_p), ("output_len", C.c_size_t),
                ("decorrelation_mode", C.c_uint8), ("split_alpha_endpoints", C.c_bool), ("split_colour_endpoints", C.c_bool),
                ("status", C.c_int32)]


@pytest.fixture(scope="module")
def ff(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, sz, b, i32 = C.c_void_p, C.c_size_t, C.c_bool, C.c_int32
    l.dxtlt_file_formats_enable_bc45.argtypes, l.dxtlt_file_formats_enable_bc45.restype = [b], None
    l.dxtlt_transform_header_pack_bc45.argtypes, l.dxtlt_transform_header_pack_bc45.restype = [i32, b], C.c_uint32
    l.dxtlt_dds_transform.argtypes, l.dxtlt_dds_transform.restype = [vp, sz, vp, sz, C.c_uint8, b, b], i32
    l.dxtlt_dds_transform_auto.argtypes = [vp, sz, vp, sz, C.POINTER(cabi.DltSizeEstimator), b]
    l.dxtlt_dds_transform_auto.restype = i32
    l.dxtlt_dds_untransform.argtypes, l.dxtlt_dds_untransform.restype = [vp, sz, vp, sz], i32
    l.dxtlt_dds_transform_batch.argtypes, l.dxtlt_dds_transform_batch.restype = [C.POINTER(DdsBatchItem), sz, b], sz
    for f in ("bc4", "bc5"):
        fn = getattr(l, f"dxtlt_transform_{f}_auto")
        fn.argtypes, fn.restype = [vp, vp, sz, C.POINTER(cabi.DltSizeEstimator), C.POINTER(b)], i32
    l.dxtlt_set_auto_estimator_threads.argtypes = [i32]
    l.dxtlt_file_formats_enable_bc45(True)
    yield l
    l.dxtlt_file_formats_enable_bc45(False)


def mip_blocks(w, h, mips):
    total = 0
    for _ in range(mips):
        total += max(1, (w + 3) // 4) * max(1, (h + 3) // 4)
        w, h = max(1, w // 2), max(1, h // 2)
    return total


def dds_file(fourcc, w, h, mips, block, rng, tail=b"", dxgi=None):
    hd = bytearray(128)
    hd[0:4] = b"DDS "
    struct.pack_into("<I", hd, 4, 124)
    struct.pack_into("<III", hd, 8, 0x1 | 0x2 | 0x4 | 0x1000 | (0x20000 if mips > 1 else 0), h, w)
    struct.pack_into("<I", hd, 0x1C, mips if mips > 1 else 0)
    struct.pack_into("<II", hd, 0x4C, 32, 0x4)
    hd[0x54:0x58] = fourcc
    if dxgi is not None:
        hd += struct.pack("<IIIII", dxgi, 3, 0, 1, 0)
    n = mip_blocks(w, h, max(1, mips))
    payload = rng.integers(0, 256, n * block, dtype=np.uint8).tobytes()
    return np.frombuffer(bytes(hd) + payload + tail, dtype=np.uint8).copy(), len(hd), n


CASES = [(b"ATI1", None, "bc4", 256, 256, 9), (b"BC4U", None, "bc4", 300, 17, 6), (b"DX10", 80, "bc4", 64, 64, 1),
         (b"ATI2", None, "bc5", 256, 256, 9), (b"BC5S", None, "bc5", 123, 45, 7), (b"DX10", 83, "bc5", 1024, 512, 11)]


@pytest.mark.parametrize("fourcc,dxgi,fmt,w,h,mips", CASES)
@pytest.mark.parametrize("split", [False, True])
def test_dds_round_trip(ff, fourcc, dxgi, fmt, w, h, mips, split):
    rng = np.random.default_rng(w * 1000 + h + mips)
    f, off, n = dds_file(fourcc, w, h, mips, bc45_ref.BLOCK[fmt], rng, tail=b"trailing bytes", dxgi=dxgi)
    out = np.zeros_like(f)
    assert ff.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, out.size, 2, split, True) == 0
    code = 8 if fmt == "bc4" else 9
    assert struct.unpack_from("<I", out.tobytes())[0] == ff.dxtlt_transform_header_pack_bc45(code, split)
    end = off + n * bc45_ref.BLOCK[fmt]
    assert np.array_equal(out[off:end], bc45_ref.transform(fmt, f[off:end], split))
    assert out[4:off].tobytes() == f[4:off].tobytes() and out[end:].tobytes() == f[end:].tobytes()
    back = np.zeros_like(f)
    assert ff.dxtlt_dds_untransform(out.ctypes.data, out.size, back.ctypes.data, back.size) == 0
    assert back.tobytes() == f.tobytes()


def test_dds_batch_round_trip(ff):
    rng = np.random.default_rng(0xDD45)
    files, fmts = [], []
    for k, (fourcc, dxgi, fmt, w, h, mips) in enumerate(CASES * 3):
        f, _, _ = dds_file(fourcc, w + k, h + 2 * k, mips, bc45_ref.BLOCK[fmt], rng, tail=bytes(k), dxgi=dxgi)
        files.append(f)
        fmts.append(fmt)
    items = (DdsBatchItem * len(files))()
    outs = [np.zeros_like(f) for f in files]
    for k, (it, f, o) in enumerate(zip(items, files, outs)):
        it.input, it.input_len, it.output, it.output_len = f.ctypes.data, f.size, o.ctypes.data, o.size
        it.split_alpha_endpoints = bool(k & 1)
    assert ff.dxtlt_dds_transform_batch(items, len(files), False) == 0
    for k, (f, o) in enumerate(zip(files, outs)):
        single = np.zeros_like(f)
        assert ff.dxtlt_dds_transform(f.ctypes.data, f.size, single.ctypes.data, single.size, 0, bool(k & 1), False) == 0
        assert o.tobytes() == single.tobytes(), k
    backs = [np.zeros_like(f) for f in files]
    for it, o, b in zip(items, outs, backs):
        it.input, it.input_len, it.output, it.output_len = o.ctypes.data, o.size, b.ctypes.data, b.size
    assert ff.dxtlt_dds_transform_batch(items, len(files), True) == 0
    for f, b in zip(files, backs):
        assert b.tobytes() == f.tobytes()


# ---- auto --------------------------------------------------------------------------------------------------------
def skewed(fmt, n, rng, flat_a0):
    """endpoint statistics that favour one setting: a0 constant and a1 random (split wins), or pairs repeating (no split wins)"""
    B = bc45_ref.BLOCK[fmt]
    x = rng.integers(0, 256, n * B, dtype=np.uint8).reshape(n, B)
    for o in ((0, 8) if fmt == "bc5" else (0,)):
        if flat_a0:
            x[:, o] = 7
        else:
            x[:, o:o + 2] = rng.integers(0, 4, (n, 1), dtype=np.uint8) * np.array([[17, 91]], dtype=np.uint8)
    return x.reshape(-1)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("threads", [1, 4])
def test_auto_picks_what_a_cpu_loop_picks(ff, fmt, threads):
    rng = np.random.default_rng(17 + threads)
    est, py_estimate = cabi.make_estimator("zlib")
    ff.dxtlt_set_auto_estimator_threads(threads)
    try:
        for k, n in enumerate([1, 129, 40_001, 300_000]):
            for flat in (False, True):
                x = skewed(fmt, n, rng, flat) if k else data(fmt, n, 3)
                want = bc45_ref.auto_choice(fmt, x, py_estimate)
                out = np.zeros_like(x)
                got = C.c_bool(not want)
                assert getattr(ff, f"dxtlt_transform_{fmt}_auto")(x.ctypes.data, out.ctypes.data, x.size, C.byref(est), C.byref(got)) == 0
                assert got.value == want, (n, flat)
                assert np.array_equal(out, bc45_ref.transform(fmt, x, want))
    finally:
        ff.dxtlt_set_auto_estimator_threads(1)
    bad, _ = cabi.make_estimator("fail_est")
    x = data(fmt, 100, 1)
    out = np.zeros_like(x)
    assert getattr(ff, f"dxtlt_transform_{fmt}_auto")(x.ctypes.data, out.ctypes.data, x.size, C.byref(bad), None) == 5


def test_dds_auto_round_trip(ff):
    rng = np.random.default_rng(5)
    est, py_estimate = cabi.make_estimator("zlib")
    for fourcc, dxgi, fmt, w, h, mips in CASES[:2] + CASES[3:5]:
        f, off, n = dds_file(fourcc, w, h, mips, bc45_ref.BLOCK[fmt], rng, dxgi=dxgi)
        end = off + n * bc45_ref.BLOCK[fmt]
        want = bc45_ref.auto_choice(fmt, f[off:end], py_estimate)
        out = np.zeros_like(f)
        assert ff.dxtlt_dds_transform_auto(f.ctypes.data, f.size, out.ctypes.data, out.size, C.byref(est), False) == 0
        assert struct.unpack_from("<I", out.tobytes())[0] == ff.dxtlt_transform_header_pack_bc45(8 if fmt == "bc4" else 9, want)
        back = np.zeros_like(f)
        assert ff.dxtlt_dds_untransform(out.ctypes.data, out.size, back.ctypes.data, back.size) == 0
        assert back.tobytes() == f.tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
def test_sharded(pkg, fmt):
    for split in (False, True):
        st = settings_of(pkg, fmt, split)
        host = data(fmt, 2_000_003, 77 + split)
        y, z = np.zeros_like(host), np.zeros_like(host)
        pkg.transform_sharded(fmt, False, host, y, st, 3)
        pkg.transform_sharded(fmt, True, y, z, st, 3)
        assert np.array_equal(y, bc45_ref.transform(fmt, host, split))
        assert np.array_equal(z, host)
