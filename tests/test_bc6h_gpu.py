"""BC6H on the MI355X: the kernels against the CPU restatement (tests/bc6h_ref.py) and by round trip, through the device, host,
range, sharded, batch, DDS and graph-captured entry points, up to a 4 GiB buffer."""
import ctypes as C
import struct

import numpy as np
import pytest

import bc6h_ref as R

pytestmark = pytest.mark.gpu

COUNTS = [1, 1023, 1024, 1025, 3 * 1024 + 7, 65_537]
MIXES = ("uniform", "single", "skewed", "raw")


def blocks_of(n, mix, seed):
    """n BC6H blocks: random bits under a mode per block -- every class evenly (uniform), one mode (single), mostly two modes
    (skewed), or raw random bytes (reserved encodings included)"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    if mix == "raw":
        return b.reshape(-1)
    codes = np.array(R.MODE_BITS + (19, 23, 27, 31), dtype=np.uint8)
    if mix == "uniform":
        k = rng.integers(0, len(codes), size=n)
    elif mix == "single":
        k = np.full(n, seed % 14)
    else:
        k = np.where(rng.random(n) < 0.9, 12, rng.choice([0, 3, 10, 14], size=n))
    mb = np.where(k <= 1, 3, 0x1F).astype(np.uint8)
    b[:, 0] = (b[:, 0] & ~mb) | codes[k]
    return b.reshape(-1)


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bc6h(pkg):
    from dxt_lossless_transform_amd import bc6h

    return bc6h


@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("n", COUNTS)
def test_device_buffers_match_reference(bc6h, dev, mix, n):
    import torch

    host = blocks_of(n, mix, n + MIXES.index(mix))
    x = torch.from_numpy(host).to(dev)
    y, z = torch.zeros_like(x), torch.zeros_like(x)
    bc6h.transform_bc6h(x, y)
    bc6h.untransform_bc6h(y, z)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), R.transform(host))
    assert torch.equal(z, x)


@pytest.mark.parametrize("off", [1, 4, 8, 20])
@pytest.mark.parametrize("n", [3, 2048, 5 * 1024 + 77])
def test_misaligned_pointers_and_guard_bytes(bc6h, dev, off, n):
    import torch

    host = blocks_of(n, "uniform", 3 * n + off)
    want = R.transform(host)
    base_in = torch.zeros(16 * n + 64, dtype=torch.uint8, device=dev)
    base_out = torch.full((16 * n + 64,), 0xA5, dtype=torch.uint8, device=dev)
    base_back = torch.full((16 * n + 64,), 0x5A, dtype=torch.uint8, device=dev)
    oo = (off * 7) % 32 + 1
    x = base_in[off:off + 16 * n]
    x.copy_(torch.from_numpy(host).to(dev))
    y = base_out[oo:oo + 16 * n]
    z = base_back[off:off + 16 * n]
    bc6h.transform_bc6h(x, y)
    bc6h.untransform_bc6h(y, z)
    torch.cuda.synchronize()
    out, back = base_out.cpu().numpy(), base_back.cpu().numpy()
    assert np.array_equal(out[oo:oo + 16 * n], want)
    assert (out[:oo] == 0xA5).all() and (out[oo + 16 * n:] == 0xA5).all()
    assert (back[:off] == 0x5A).all() and (back[off + 16 * n:] == 0x5A).all()
    assert torch.equal(z, x)


@pytest.mark.parametrize("n", [1, 1025, 70_001, 7_000_003])
def test_host_buffers(bc6h, n):
    host = blocks_of(n, "skewed", n)
    y, z = np.zeros_like(host), np.zeros_like(host)
    bc6h.transform_bc6h(host, y)
    bc6h.untransform_bc6h(y, z)
    assert np.array_equal(z, host)
    if n <= 70_001:
        assert np.array_equal(y, R.transform(host))
    else:
        main = n - n % 1024   # granule 1000, checked against the reference through its slice of every stream
        part = R.transform(host[16 * 1024 * 1000:16 * 1024 * 1001])
        for o, w in zip(R.STREAM_OFF, R.STREAM_WIDTH):
            start = o * main + w * 1024 * 1000
            assert np.array_equal(y[start:start + w * 1024], part[o * 1024:(o + w) * 1024]), o


def test_ranges_compose(bc6h, dev):
    import torch

    from dxt_lossless_transform_amd import DeviceError

    n = 7 * 1024 + 300
    host = blocks_of(n, "uniform", 17)
    x = torch.from_numpy(host).to(dev)
    whole = torch.zeros_like(x)
    bc6h.transform_bc6h(x, whole)
    cuts = [0, 1024, 4096, 5120, n]
    soa = torch.zeros_like(x)
    for a, b in zip(cuts, cuts[1:]):
        bc6h.transform_bc6h_range(False, x[16 * a:16 * b], soa, n, a, b - a)
    back = torch.zeros_like(x)
    for a, b in zip(cuts, cuts[1:]):
        bc6h.transform_bc6h_range(True, soa, back[16 * a:16 * b], n, a, b - a)
    torch.cuda.synchronize()
    assert torch.equal(soa, whole)
    assert torch.equal(back, x)
    with pytest.raises(DeviceError):
        bc6h.transform_bc6h_range(False, x[16 * 100:], soa, n, 100, 1024)
    with pytest.raises(DeviceError):
        bc6h.transform_bc6h_range(False, x, soa, n, 0, 1000)


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_sharded_equals_unsharded(bc6h, shards):
    n = 9 * 1024 + 5
    host = blocks_of(n, "uniform", 100 + shards)
    one, many, back = np.zeros_like(host), np.zeros_like(host), np.zeros_like(host)
    bc6h.transform_bc6h(host, one)
    bc6h.transform_bc6h_sharded(host, many, shards)
    bc6h.transform_bc6h_sharded(many, back, shards, inverse=True)
    assert np.array_equal(many, one)
    assert np.array_equal(back, host)


def test_mixed_batch_equals_single_calls(pkg, bc6h, dev, oracle):
    import torch

    from dxt_lossless_transform_amd import batch, bc7

    rng = np.random.default_rng(0xBA6)
    plan = []
    for k in range(18):
        fmt = ("bc1", "bc6h", "bc7")[k % 3]
        n = int(rng.choice([1, 1023, 4096, 5 * 1024 + 3, int(rng.integers(1, 100_000))]))
        inverse = bool(k % 4 == 3) and fmt != "bc7"
        B = 8 if fmt == "bc1" else 16
        host = rng.integers(0, 256, n * B, dtype=np.uint8)
        if fmt == "bc7":
            oracle.bc7_force_modes(host)
        elif fmt == "bc6h":
            host = blocks_of(n, "uniform", k)
        st = pkg.Bc1TransformSettings() if fmt == "bc1" else None
        plan.append((fmt, inverse, host, st))
    items, outs, want = [], [], []
    for fmt, inverse, host, st in plan:
        x = torch.from_numpy(host).to(dev)
        y, ref = torch.zeros_like(x), torch.zeros_like(x)
        if fmt == "bc7":
            (bc7.untransform_bc7 if inverse else bc7.transform_bc7)(x, ref)
        elif fmt == "bc6h":
            (bc6h.untransform_bc6h if inverse else bc6h.transform_bc6h)(x, ref)
        else:
            getattr(pkg, f"{'untransform' if inverse else 'transform'}_bc1_with_settings")(x, ref, st)
        items.append((fmt, inverse, x, y, st))
        outs.append(y)
        want.append(ref)
    batch.transform_batch(items)
    torch.cuda.synchronize()
    for (fmt, inverse, host, st), y, ref in zip(plan, outs, want):
        assert torch.equal(y, ref), (fmt, inverse, host.size)
        if fmt == "bc6h":
            assert np.array_equal(y.cpu().numpy(), (R.untransform if inverse else R.transform)(host))
    host_items, host_outs = [], []
    for fmt, inverse, host, st in plan:
        o = np.zeros_like(host)
        host_items.append((fmt, inverse, host, o, st))
        host_outs.append(o)
    batch.transform_batch_host(host_items)
    for o, ref in zip(host_outs, want):
        assert np.array_equal(o, ref.cpu().numpy())


# ---- DDS ---------------------------------------------------------------------------------------------------------------
class DdsBatchItem(C.Structure):
    _fields_ = [("input", C.c_void_p), ("input_len", C.c_size_t), ("output", C.c_void_p), ("output_len", C.c_size_t),
                ("decorrelation_mode", C.c_uint8), ("split_alpha_endpoints", C.c_bool), ("split_colour_endpoints", C.c_bool),
                ("status", C.c_int32)]


@pytest.fixture(scope="module")
def ff(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, sz, b, i32 = C.c_void_p, C.c_size_t, C.c_bool, C.c_int32
    l.dxtlt_file_formats_enable_bc6h.argtypes, l.dxtlt_file_formats_enable_bc6h.restype = [b], None
    l.dxtlt_dds_transform.argtypes, l.dxtlt_dds_transform.restype = [vp, sz, vp, sz, C.c_uint8, b, b], i32
    l.dxtlt_dds_untransform.argtypes, l.dxtlt_dds_untransform.restype = [vp, sz, vp, sz], i32
    l.dxtlt_dds_transform_batch.argtypes, l.dxtlt_dds_transform_batch.restype = [C.POINTER(DdsBatchItem), sz, b], sz
    l.dxtlt_file_formats_enable_bc6h(True)
    yield l
    l.dxtlt_file_formats_enable_bc6h(False)


def mip_blocks(w, h, mips):
    total = 0
    for _ in range(mips):
        total += max(1, (w + 3) // 4) * max(1, (h + 3) // 4)
        w, h = max(1, w // 2), max(1, h // 2)
    return total


def dds_file(w, h, mips, dxgi, seed):
    n = mip_blocks(w, h, mips)
    payload = blocks_of(n, "uniform", seed).tobytes()
    f = np.frombuffer(R.dds_dx10(payload, w, h, dxgi, mips) + b"trailing bytes", dtype=np.uint8).copy()
    return f, 148, n


@pytest.mark.parametrize("dxgi,w,h,mips", [(95, 256, 256, 9), (96, 300, 17, 6), (94, 1024, 512, 11), (96, 4, 4, 1)])
def test_dds_round_trip(ff, dxgi, w, h, mips):
    f, off, n = dds_file(w, h, mips, dxgi, w + h + mips)
    out = np.zeros_like(f)
    assert ff.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, out.size, 2, True, True) == 0
    assert struct.unpack_from("<I", out.tobytes())[0] == R.HEADER_WORD
    end = off + 16 * n
    assert np.array_equal(out[off:end], R.transform(f[off:end]))
    assert out[4:off].tobytes() == f[4:off].tobytes() and out[end:].tobytes() == f[end:].tobytes()
    back = np.zeros_like(f)
    assert ff.dxtlt_dds_untransform(out.ctypes.data, out.size, back.ctypes.data, back.size) == 0
    assert back.tobytes() == f.tobytes()


def test_dds_batch_round_trip(ff):
    files = [dds_file(w, h, m, dxgi, i)[0] for i, (dxgi, w, h, m) in
             enumerate([(95, 128, 128, 8), (96, 64, 32, 3), (95, 2048, 2048, 1), (96, 12, 12, 2)])]
    singles = []
    for f in files:
        o = np.zeros_like(f)
        assert ff.dxtlt_dds_transform(f.ctypes.data, f.size, o.ctypes.data, o.size, 0, False, False) == 0
        singles.append(o)
    items = (DdsBatchItem * len(files))()
    outs = [np.zeros_like(f) for f in files]
    for it, f, o in zip(items, files, outs):
        it.input, it.input_len, it.output, it.output_len, it.status = f.ctypes.data, f.size, o.ctypes.data, o.size, -1
    assert ff.dxtlt_dds_transform_batch(items, len(files), False) == 0
    for o, s in zip(outs, singles):
        assert o.tobytes() == s.tobytes()
    backs = [np.zeros_like(f) for f in files]
    for it, o, b in zip(items, outs, backs):
        it.input, it.input_len, it.output, it.output_len, it.status = o.ctypes.data, o.size, b.ctypes.data, b.size, -1
    assert ff.dxtlt_dds_transform_batch(items, len(files), True) == 0
    for b, f in zip(backs, files):
        assert b.tobytes() == f.tobytes()


# ---- graph capture and size -------------------------------------------------------------------------------------------
def test_graph_capture_replays(bc6h, dev):
    import torch

    n = 5 * 1024 + 77                     # main part + tail part: two launches per direction
    x = torch.from_numpy(blocks_of(n, "uniform", 1)).to(dev)
    y, z = torch.zeros_like(x), torch.zeros_like(x)

    def work():
        bc6h.transform_bc6h(x, y)
        bc6h.untransform_bc6h(y, z)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    fresh = blocks_of(n, "skewed", 2)
    x.copy_(torch.from_numpy(fresh))
    y.zero_()
    z.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(y.cpu().numpy(), R.transform(fresh))
    assert np.array_equal(z.cpu().numpy(), fresh)


def test_4gib_round_trip_with_sampled_granules(bc6h, dev):
    import torch

    n = (4 << 30) // 16
    g = torch.Generator(device=dev)
    g.manual_seed(0xBC6)
    x = torch.randint(0, 256, (16 * n,), dtype=torch.uint8, device=dev, generator=g)
    codes = torch.tensor(list(R.MODE_BITS) + [19], dtype=torch.uint8, device=dev)
    k = torch.randint(0, len(codes), (n,), device=dev, generator=g)
    b0 = x.view(n, 16)[:, 0]
    mb = torch.where(k <= 1, 3, 0x1F).to(torch.uint8)
    b0.copy_((b0 & ~mb) | codes[k])
    y = torch.empty_like(x)
    bc6h.transform_bc6h(x, y)
    z = torch.empty_like(x)
    bc6h.untransform_bc6h(y, z)
    torch.cuda.synchronize()
    assert torch.equal(z, x)
    del z
    main = n - n % 1024
    for gi in (0, 1, 177_777, main // 1024 - 1):
        blocks = x[16 * 1024 * gi:16 * 1024 * (gi + 1)].cpu().numpy()
        part = R.transform(blocks)
        for o, w in zip(R.STREAM_OFF, R.STREAM_WIDTH):
            got = y[o * main + w * 1024 * gi:o * main + w * 1024 * (gi + 1)].cpu().numpy()
            assert np.array_equal(got, part[o * 1024:(o + w) * 1024]), (gi, o)
