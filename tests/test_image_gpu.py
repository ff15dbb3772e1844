"""Image decoders on the MI355X (include/dxtlt_image.h): the fused untransform + decode call and the plain image decoder
against the CPU statement -- oracle_c.decode_blocks rearranged into rows -- with exact equality everywhere.  Every output
sits inside guard bytes and is prefilled with 0xA5: the guards, the pitch padding and the bytes behind the last row's pixels
must still be 0xA5 afterwards.  The largest image is 1026 x 9 pixels."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 128   # a payload at offset 0 stays on a 128-byte line: the aligned tiles' condition
OK = 0
FMTS = ("bc1", "bc2", "bc3")
FMT_ID = {"bc1": 1, "bc2": 2, "bc3": 3}
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16}
DEFAULT = (1, True, True)   # decorrelation mode (core numbering), split alpha, split colour: the settings types' defaults
SHAPES = [(1, 1), (2, 3), (4, 4), (5, 7), (20, 9), (256, 4), (260, 8), (1026, 9), (1024, 8)]


def all_settings(fmt):
    """every (variant, split alpha, split colour): 8 / 8 / 16"""
    return [(v, sa, sc) for v in range(4) for sa in ((False, True) if fmt == "bc3" else (False,)) for sc in (False, True)]


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, i32, u32, u64, u8, b = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint8, C.c_bool
    l.dxtlt_decode_image_device.argtypes = [i32, vp, u32, u32, vp, u64, vp]
    l.dxtlt_untransform_decode_image_device.argtypes = [i32, vp, u64, u64, u32, u32, u8, b, b, vp, u64, vp]
    l.dxtlt_untransform_decode_image.argtypes = [i32, vp, C.c_size_t, u64, u32, u32, u8, b, b, vp, u64]
    for f in (l.dxtlt_decode_image_device, l.dxtlt_untransform_decode_image_device, l.dxtlt_untransform_decode_image):
        f.restype = i32
    l.dxtlt_debug_plan_transform.argtypes = [i32, i32, i32, i32, i32, u64, u64, u64, u64, u64, C.POINTER(PlannedLaunch), i32]
    l.dxtlt_debug_plan_transform.restype = i32
    return l


class PlannedLaunch(C.Structure):   # DxtltDebugPlannedLaunch, include/dxtlt_gfx950.h
    _fields_ = [("kind", C.c_int32), ("threads", C.c_int32), ("workgroups", C.c_uint32), ("full_tiles", C.c_uint32),
                ("range_blocks", C.c_uint64), ("aos_offset", C.c_uint64), ("shift", C.c_uint8 * 6), ("halo_vecs", C.c_uint8),
                ("natural", C.c_uint8), ("gbase", C.c_uint64 * 6)]


def planned_kinds(lib, fmt, settings, address, total, first, num):
    """the tile kinds the inverse direction takes for a range at this transformed-side address (0 aligned, 2 shifted / edge)"""
    out = (PlannedLaunch * 8)()
    n = lib.dxtlt_debug_plan_transform(FMT_ID[fmt], 1, settings[0], settings[1], settings[2], address, 0, total, first, num, out, 8)
    assert 0 < n <= 8
    return [out[i].kind for i in range(n)]


def blocks_of(width, height):
    return ((width + 3) // 4) * ((height + 3) // 4)


@functools.lru_cache(maxsize=None)
def random_blocks(fmt, n, seed=0):
    """seeded random blocks; every 7th with colour endpoints c0 <= c1 (every 21st c0 == c1): BC1's three-colour mode and equal
    endpoints; random BC3 alpha endpoints are a0 <= a1 (the six-value table) in half of the blocks, a0 == a1 in every 35th"""
    bs = BLOCK[fmt]
    x = np.random.default_rng(0x1A6E + 131 * n + FMT_ID[fmt] + 7919 * seed).integers(0, 256, n * bs, dtype=np.uint8).reshape(n, bs)
    at = 0 if fmt == "bc1" else 8
    c = x[:, at:at + 4].copy().view("<u2")            # (n, 2): c0, c1
    lo, hi = c.min(axis=1), c.max(axis=1)
    c[::7, 0], c[::7, 1] = lo[::7], hi[::7]
    c[::21, 1] = c[::21, 0]
    x[:, at:at + 4] = c.view(np.uint8)
    if fmt == "bc3":
        x[::35, 1] = x[::35, 0]
    x.setflags(write=False)
    return x.reshape(-1)


def image_of(oracle, fmt, blocks, width, height):
    """the expected height x width x 4 image of a block array in block order"""
    bx, by = (width + 3) // 4, (height + 3) // 4
    px = oracle.decode_blocks(fmt, blocks).reshape(by, bx, 4, 4, 4)   # block row, block column, pixel row, pixel column, rgba
    return np.ascontiguousarray(px.transpose(0, 2, 1, 3, 4).reshape(4 * by, 4 * bx, 4)[:height, :width])


_cache = {}


def reference(oracle, fmt, n, settings=DEFAULT, seed=0):
    """(blocks, transformed) of a whole array of n blocks, computed once per case and shared"""
    key = (fmt, n, settings, seed)
    if key not in _cache:
        x = random_blocks(fmt, n, seed)
        t = oracle.transform(fmt, x, settings[0], settings[2], settings[1])
        t.setflags(write=False)
        _cache[key] = (x, t)
    return _cache[key]


class Guarded:
    """`n` device bytes at offset `off` from a 256-byte aligned address, GUARD + off bytes of 0xA5 in front and GUARD behind"""

    def __init__(self, dev, n, off=0, data=None):
        import torch

        self.n, self.at = n, GUARD + off
        self.base = torch.full((self.at + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert self.base.data_ptr() % 256 == 0
        if data is not None:
            self.base[self.at:self.at + n].copy_(torch.from_numpy(np.array(data, copy=True)).to(dev))
        self.ptr = self.base.data_ptr() + self.at
        self.view = self.base[self.at:self.at + n]

    def bytes(self):
        """the payload, after checking the guards"""
        host = self.base.cpu().numpy()
        assert (host[:self.at] == 0xA5).all() and (host[self.at + self.n:] == 0xA5).all(), "guard bytes were written"
        return host[self.at:self.at + self.n]


def expected_buffer(image, pitch):
    """pitch * height bytes: the image's rows, 0xA5 everywhere else"""
    height, width = image.shape[:2]
    want = np.full((height, pitch), 0xA5, dtype=np.uint8)
    want[:, :4 * width] = image.reshape(height, 4 * width)
    return want.reshape(-1)


def run_fused(lib, dev, fmt, transformed, total, first, width, height, settings, pitch=None, out_off=0, in_off=0):
    import torch

    pitch = 4 * width if pitch is None else pitch
    src = Guarded(dev, transformed.size, in_off, transformed)
    dst = Guarded(dev, pitch * height, out_off)
    with torch.cuda.device(dev):
        rc = lib.dxtlt_untransform_decode_image_device(FMT_ID[fmt], src.ptr, total, first, width, height, settings[0], settings[1],
                                                       settings[2], dst.ptr, pitch, torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), transformed), "the transformed buffer changed"
    return dst.bytes()


def run_plain(lib, dev, fmt, blocks, width, height, pitch=None, out_off=0, in_off=0):
    import torch

    pitch = 4 * width if pitch is None else pitch
    src = Guarded(dev, blocks.size, in_off, blocks)
    dst = Guarded(dev, pitch * height, out_off)
    with torch.cuda.device(dev):
        rc = lib.dxtlt_decode_image_device(FMT_ID[fmt], src.ptr, width, height, dst.ptr, pitch, torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), blocks), "the block array changed"
    return dst.bytes()


# ---- case 1: every setting ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1026, 9), (20, 9)])
@pytest.mark.parametrize("fmt", FMTS)
def test_fused_call_with_every_setting(lib, dev, oracle, fmt, shape):
    width, height = shape
    n = blocks_of(width, height)
    combos = all_settings(fmt)
    assert len(combos) == (16 if fmt == "bc3" else 8)
    want = None
    for settings in combos:
        x, t = reference(oracle, fmt, n, settings)
        if want is None:
            want = expected_buffer(image_of(oracle, fmt, x, width, height), 4 * width)
        got = run_fused(lib, dev, fmt, t, n, 0, width, height, settings)
        assert np.array_equal(got, want), (fmt, shape, settings)


# ---- case 2: every shape -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_pitch", [0, 20])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_shape_fused_and_plain(lib, dev, oracle, fmt, shape, extra_pitch):
    width, height = shape
    n = blocks_of(width, height)
    pitch = 4 * width + extra_pitch
    x, t = reference(oracle, fmt, n)
    want = expected_buffer(image_of(oracle, fmt, x, width, height), pitch)
    if shape == (1024, 8):
        assert planned_kinds(lib, fmt, DEFAULT, 256, n, 0, n) == [0]           # whole aligned tiles, nothing else
    assert np.array_equal(run_fused(lib, dev, fmt, t, n, 0, width, height, DEFAULT, pitch), want), "fused"
    assert np.array_equal(run_plain(lib, dev, fmt, x, width, height, pitch), want), "plain"


# ---- case 3: ranges ----------------------------------------------------------------------------------------------------
def mip_chain(width, height, mip_count):
    levels, first = [], 0
    for k in range(mip_count):
        w, h = max(1, width >> k), max(1, height >> k)
        levels.append((w, h, first, blocks_of(w, h)))
        first += levels[-1][3]
    return levels, first


@pytest.mark.parametrize("settings", ["default", "other"])
@pytest.mark.parametrize("fmt", FMTS)
def test_levels_of_a_transformed_mip_chain(lib, dev, oracle, fmt, settings):
    settings = DEFAULT if settings == "default" else (3, False, False) if fmt != "bc3" else (2, True, False)
    levels, total = mip_chain(256, 256, 9)
    assert total == 5463 and [levels[k][2] for k in (1, 3, 6)] == [4096, 5376, 5460]
    assert planned_kinds(lib, fmt, settings, 256, total, 0, 4096) == [2]       # an odd total: shifted tiles
    x, t = reference(oracle, fmt, total, settings)
    bs = BLOCK[fmt]
    for k in (0, 1, 3, 6, 7, 8):
        w, h, first, num = levels[k]
        want = expected_buffer(image_of(oracle, fmt, x[first * bs:(first + num) * bs], w, h), 4 * w)
        got = run_fused(lib, dev, fmt, t, total, first, w, h, settings)
        assert np.array_equal(got, want), (fmt, settings, k)


@pytest.mark.parametrize("fmt", FMTS)
def test_range_whose_stream_bases_are_on_128_byte_lines(lib, dev, oracle, fmt):
    total, first = 8192, 4096
    x, t = reference(oracle, fmt, total)
    bs = BLOCK[fmt]
    # 128 x 128: whole aligned tiles; 132 x 128 (33 blocks per row): aligned tiles and an edge tile behind them, in a launch of its own
    for width, height, kinds in ((128, 128, [0]), (132, 128, [0, 2])):
        num = blocks_of(width, height)
        assert planned_kinds(lib, fmt, DEFAULT, 256, total, first, num) == kinds   # (a guarded payload sits on a 128-byte line)
        want = expected_buffer(image_of(oracle, fmt, x[first * bs:(first + num) * bs], width, height), 4 * width)
        assert np.array_equal(run_fused(lib, dev, fmt, t, total, first, width, height, DEFAULT), want), (width, height)


# ---- case 4: alignment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(260, 8), (1026, 9)])
@pytest.mark.parametrize("fmt", FMTS)
def test_pointer_alignments(lib, dev, oracle, fmt, shape):
    width, height = shape
    n = blocks_of(width, height)
    x, t = reference(oracle, fmt, n)
    want = expected_buffer(image_of(oracle, fmt, x, width, height), 4 * width)
    for out_off in (4, 8, 12):
        assert np.array_equal(run_fused(lib, dev, fmt, t, n, 0, width, height, DEFAULT, out_off=out_off), want), ("fused", out_off)
        assert np.array_equal(run_plain(lib, dev, fmt, x, width, height, out_off=out_off), want), ("plain", out_off)
    assert np.array_equal(run_plain(lib, dev, fmt, x, width, height, in_off=1), want), "plain, blocks at offset 1"
    for in_off in (1, 8):
        assert np.array_equal(run_fused(lib, dev, fmt, t, n, 0, width, height, DEFAULT, in_off=in_off), want), ("fused", in_off)


# ---- case 5: the three routes agree ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_fused_plain_and_host_calls_agree(lib, dev, oracle, fmt):
    width, height = 1026, 9
    n = blocks_of(width, height)
    pitch = 4 * width + 20
    x, t = reference(oracle, fmt, n)
    want = expected_buffer(image_of(oracle, fmt, x, width, height), pitch)
    fused = run_fused(lib, dev, fmt, t, n, 0, width, height, DEFAULT, pitch)
    plain = run_plain(lib, dev, fmt, x, width, height, pitch)
    host = np.full(GUARD + pitch * height + GUARD, 0xA5, dtype=np.uint8)
    rc = lib.dxtlt_untransform_decode_image(FMT_ID[fmt], t.ctypes.data, t.size, 0, width, height, DEFAULT[0], DEFAULT[1], DEFAULT[2],
                                            host.ctypes.data + GUARD, pitch)
    assert rc == OK
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + pitch * height:] == 0xA5).all()
    host = host[GUARD:GUARD + pitch * height]
    assert np.array_equal(fused, want) and np.array_equal(plain, fused) and np.array_equal(host, fused)


def test_python_module_on_tensors_and_host_buffers(pkg, dev, oracle):
    import torch

    from dxt_lossless_transform_amd import image

    levels, total = mip_chain(256, 256, 9)
    w, h, first, num = levels[3]
    assert image.mip_level(256, 256, 9, 3) == (w, h, first, num, total)
    for fmt in FMTS:
        x, t = reference(oracle, fmt, total)
        bs = BLOCK[fmt]
        want = image_of(oracle, fmt, x[first * bs:(first + num) * bs], w, h).reshape(-1)
        kw = dict(first_block=first, decorrelation_mode=pkg.YCoCgVariant.Variant1, split_alpha_endpoints=True,
                  split_colour_endpoints=True)
        got = image.untransform_decode_image(fmt, torch.from_numpy(t.copy()).to(dev), w, h, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(image.untransform_decode_image(fmt, t, w, h, **kw), want)
        got = image.decode_image(fmt, torch.from_numpy(x[first * bs:(first + num) * bs].copy()).to(dev), w, h)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)


# ---- case 6: graph capture ---------------------------------------------------------------------------------------------
def test_fused_call_replays_from_a_hip_graph(lib, dev, oracle):
    import torch

    fmt, width, height = "bc3", 1026, 9
    n = blocks_of(width, height)
    x, t = reference(oracle, fmt, n)
    src = Guarded(dev, t.size, 0, t)
    dst = Guarded(dev, 4 * width * height)

    def work():
        rc = lib.dxtlt_untransform_decode_image_device(FMT_ID[fmt], src.ptr, n, 0, width, height, DEFAULT[0], DEFAULT[1], DEFAULT[2],
                                                       dst.ptr, 4 * width, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == OK

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        work()                                    # warm-up outside capture (module load, first launch)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    # new blocks in the same buffer, the output cleared: only a replay can produce the right image now
    x2, t2 = reference(oracle, fmt, n, DEFAULT, seed=1)
    assert not np.array_equal(x, x2)
    src.view.copy_(torch.from_numpy(t2.copy()).to(dev))
    dst.view.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(dst.bytes(), expected_buffer(image_of(oracle, fmt, x2, width, height), 4 * width))
    assert np.array_equal(src.bytes(), t2)
