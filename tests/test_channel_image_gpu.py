"""BC4 / BC5 image decoders on the MI355X (include/dxtlt_image.h, the *_channel_image calls): the fused untransform + decode
call and the plain image decoder against the CPU statement of tests/channel_image_ref.py -- the oracle's BC3 alpha channel of
every 8-byte half, rearranged into rows -- with exact equality everywhere.  Every output sits inside guard bytes and is
prefilled with 0xA5: the guards, the pitch padding and the bytes behind the last row's pixels must still be 0xA5 afterwards,
and the source is unchanged.  The largest image is 1026 x 9 pixels, except the one 1024 x 1024 case."""
import ctypes as C

import numpy as np
import pytest

import bc45_ref
import channel_image_ref as ref
from channel_image_ref import BLOCK, BPP, FMT_ID, blocks_of, expected_buffer, image_of

pytestmark = pytest.mark.gpu

GUARD = 256   # a payload at offset 0 stays on a 256-byte address
OK = 0
FMTS = ("bc4", "bc5")
SHAPES = [(1, 1), (2, 3), (4, 4), (5, 7), (13, 5), (16, 4), (20, 9), (28, 8), (260, 8), (1024, 8), (1026, 9)]
EXTRA_PITCH = {"bc4": (0, 1, 20), "bc5": (0, 2, 20)}


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


class PlannedLaunch(C.Structure):   # DxtltDebugPlannedLaunch, include/dxtlt_gfx950.h
    _fields_ = [("kind", C.c_int32), ("threads", C.c_int32), ("workgroups", C.c_uint32), ("full_tiles", C.c_uint32),
                ("range_blocks", C.c_uint64), ("aos_offset", C.c_uint64), ("shift", C.c_uint8 * 6), ("halo_vecs", C.c_uint8),
                ("natural", C.c_uint8), ("gbase", C.c_uint64 * 6)]


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, i32, u32, u64, b = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_bool
    l.dxtlt_decode_channel_image_device.argtypes = [i32, vp, u32, u32, vp, u64, vp]
    l.dxtlt_untransform_decode_channel_image_device.argtypes = [i32, vp, u64, u64, u32, u32, b, vp, u64, vp]
    l.dxtlt_untransform_decode_channel_image.argtypes = [i32, vp, C.c_size_t, u64, u32, u32, b, vp, u64]
    l.dxtlt_image_mip_level.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64),
                                        C.POINTER(u64)]
    for f in (l.dxtlt_decode_channel_image_device, l.dxtlt_untransform_decode_channel_image_device,
              l.dxtlt_untransform_decode_channel_image, l.dxtlt_image_mip_level):
        f.restype = i32
    l.dxtlt_debug_plan_transform.argtypes = [i32, i32, i32, i32, i32, u64, u64, u64, u64, u64, C.POINTER(PlannedLaunch), i32]
    l.dxtlt_debug_plan_transform.restype = i32
    return l


def planned_kinds(lib, fmt, split, address, total, first, num):
    """the tile kinds the inverse direction takes for a range at this transformed-side address (0 aligned, 2 shifted / edge)"""
    out = (PlannedLaunch * 8)()
    n = lib.dxtlt_debug_plan_transform(FMT_ID[fmt], 1, 0, int(split), 0, address, 0, total, first, num, out, 8)
    assert 0 < n <= 8
    return [out[i].kind for i in range(n)]


_cache = {}


def reference(fmt, n, split, seed=0):
    """(blocks, transformed) of a whole array of n blocks, computed once per case and shared"""
    key = (fmt, n, split, seed)
    if key not in _cache:
        x = ref.random_blocks(fmt, n, seed)
        t = bc45_ref.transform(fmt, x, split)
        t.setflags(write=False)
        _cache[key] = (x, t)
    return _cache[key]


_images = {}


def expected(oracle, fmt, n, width, height, pitch, seed=0, first=0):
    """the expected output buffer for blocks [first, first + blocks of the image) of random_blocks(fmt, n, seed), shared"""
    key = (fmt, n, width, height, seed, first)
    if key not in _images:
        bs = BLOCK[fmt]
        x = ref.random_blocks(fmt, n, seed)[first * bs:(first + blocks_of(width, height)) * bs]
        _images[key] = image_of(oracle, fmt, x, width, height)
    return expected_buffer(_images[key], pitch)


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


def run_fused(lib, dev, fmt, transformed, total, first, width, height, split, pitch=None, out_off=0, in_off=0):
    import torch

    pitch = BPP[fmt] * width if pitch is None else pitch
    src = Guarded(dev, transformed.size, in_off, transformed)
    dst = Guarded(dev, pitch * height, out_off)
    with torch.cuda.device(dev):
        rc = lib.dxtlt_untransform_decode_channel_image_device(FMT_ID[fmt], src.ptr, total, first, width, height, split, dst.ptr,
                                                               pitch, torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), transformed), "the transformed buffer changed"
    return dst.bytes()


def run_plain(lib, dev, fmt, blocks, width, height, pitch=None, out_off=0, in_off=0):
    import torch

    pitch = BPP[fmt] * width if pitch is None else pitch
    src = Guarded(dev, blocks.size, in_off, blocks)
    dst = Guarded(dev, pitch * height, out_off)
    with torch.cuda.device(dev):
        rc = lib.dxtlt_decode_channel_image_device(FMT_ID[fmt], src.ptr, width, height, dst.ptr, pitch,
                                                   torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), blocks), "the block array changed"
    return dst.bytes()


# ---- case 1: both settings x every shape x fused and plain -------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_shape_fused_and_plain(lib, dev, oracle, fmt, shape, split):
    width, height = shape
    n = blocks_of(width, height)
    x, t = reference(fmt, n, split)
    if shape == (1024, 8):
        assert planned_kinds(lib, fmt, split, 256, n, 0, n) == [0]             # whole aligned tiles, nothing else
    if shape == (1026, 9):
        assert 2 in planned_kinds(lib, fmt, split, 256, n, 0, n)
    for extra in EXTRA_PITCH[fmt]:
        pitch = BPP[fmt] * width + extra
        want = expected(oracle, fmt, n, width, height, pitch)
        assert np.array_equal(run_fused(lib, dev, fmt, t, n, 0, width, height, split, pitch), want), ("fused", extra)
        assert np.array_equal(run_plain(lib, dev, fmt, x, width, height, pitch), want), ("plain", extra)


# ---- case 2: every endpoint pair ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_every_endpoint_pair_on_the_device(lib, dev, oracle, fmt):
    """the 65 536 BC4 blocks of the layout test as a 1024 x 1024 image; the same bytes as 32 768 BC5 blocks, 1024 x 512"""
    x = ref.every_endpoint_pair()
    width, height, split = (1024, 1024, False) if fmt == "bc4" else (1024, 512, True)
    n = blocks_of(width, height)
    assert n * BLOCK[fmt] == x.size
    want = expected_buffer(image_of(oracle, fmt, x, width, height), BPP[fmt] * width)
    t = bc45_ref.transform(fmt, x, split)
    assert np.array_equal(run_fused(lib, dev, fmt, t, n, 0, width, height, split), want), "fused"
    assert np.array_equal(run_plain(lib, dev, fmt, x, width, height), want), "plain"


# ---- case 3: ranges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_ranges_at_every_group_phase(lib, dev, oracle, fmt, split):
    width, height = 20, 9
    num = blocks_of(width, height)
    assert num == 15
    for first in range(9):
        for tail in (0, 1, 5):
            total = first + num + tail
            x, t = reference(fmt, total, split)
            want = expected(oracle, fmt, total, width, height, BPP[fmt] * width, first=first)
            got = run_fused(lib, dev, fmt, t, total, first, width, height, split)
            assert np.array_equal(got, want), (first, total)


def mip_level(lib, width, height, mip_count, level):
    w, h = C.c_uint32(), C.c_uint32()
    first, num, total = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.dxtlt_image_mip_level(width, height, mip_count, level, C.byref(w), C.byref(h), C.byref(first), C.byref(num),
                                     C.byref(total)) == OK
    return w.value, h.value, first.value, num.value, total.value


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_levels_of_a_transformed_mip_chain(lib, dev, oracle, fmt, split):
    levels = [mip_level(lib, 40, 24, 6, k) for k in range(6)]
    assert [l[3] for l in levels] == [60, 15, 6, 2, 1, 1] and [l[2] for l in levels] == [0, 60, 75, 81, 83, 84]
    total = levels[0][4]
    assert total == 85
    x, t = reference(fmt, total, split)
    for k, (w, h, first, num, _) in enumerate(levels):
        want = expected(oracle, fmt, total, w, h, BPP[fmt] * w, first=first)
        assert np.array_equal(run_fused(lib, dev, fmt, t, total, first, w, h, split), want), k


# ---- case 4: alignment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(260, 8), (1026, 9)])
@pytest.mark.parametrize("fmt", FMTS)
def test_pointer_alignments(lib, dev, oracle, fmt, shape):
    width, height = shape
    n = blocks_of(width, height)
    split = fmt == "bc5"
    x, t = reference(fmt, n, split)
    row = BPP[fmt] * width
    # 260: BC4 260 (not a multiple of 16), BC5 520; with 12 more BC4 272 = 16 * 17, and 1026: BC5 2052, with 12 more 2064 = 16 * 129
    pitches = sorted({row, row + 12, (row + 15) // 16 * 16})
    assert any(p % 16 == 0 for p in pitches) and any(p % 16 != 0 for p in pitches)
    for pitch in pitches:
        want = expected(oracle, fmt, n, width, height, pitch)
        for out_off in ((0, 1, 2, 3, 4, 8) if fmt == "bc4" else (0, 2, 4, 8)):
            assert np.array_equal(run_fused(lib, dev, fmt, t, n, 0, width, height, split, pitch, out_off=out_off), want), \
                ("fused", pitch, out_off)
            assert np.array_equal(run_plain(lib, dev, fmt, x, width, height, pitch, out_off=out_off), want), ("plain", pitch, out_off)
    want = expected(oracle, fmt, n, width, height, row)
    for in_off in (0, 1, 8, 16, 64):
        assert np.array_equal(run_fused(lib, dev, fmt, t, n, 0, width, height, split, in_off=in_off), want), ("fused", in_off)
        assert np.array_equal(run_plain(lib, dev, fmt, x, width, height, in_off=in_off), want), ("plain", in_off)


# ---- case 5: the three routes agree ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_fused_plain_and_host_calls_agree(lib, dev, oracle, fmt):
    width, height, split = 1026, 9, True
    n = blocks_of(width, height)
    pitch = BPP[fmt] * width + 20
    x, t = reference(fmt, n, split)
    want = expected(oracle, fmt, n, width, height, pitch)
    fused = run_fused(lib, dev, fmt, t, n, 0, width, height, split, pitch)
    plain = run_plain(lib, dev, fmt, x, width, height, pitch)
    host = np.full(GUARD + pitch * height + GUARD, 0xA5, dtype=np.uint8)
    rc = lib.dxtlt_untransform_decode_channel_image(FMT_ID[fmt], t.ctypes.data, t.size, 0, width, height, split,
                                                    host.ctypes.data + GUARD, pitch)
    assert rc == OK
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + pitch * height:] == 0xA5).all()
    host = host[GUARD:GUARD + pitch * height]
    assert np.array_equal(fused, want) and np.array_equal(plain, fused) and np.array_equal(host, fused)


# ---- case 6: the Python module -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_python_module_on_tensors_and_host_buffers(pkg, lib, dev, oracle, fmt):
    import torch

    from dxt_lossless_transform_amd import image

    w, h, first, num, total = image.mip_level(40, 24, 6, 1)
    bs, split = BLOCK[fmt], fmt == "bc4"
    x, t = reference(fmt, total, split)
    want = expected(oracle, fmt, total, w, h, BPP[fmt] * w, first=first)
    kw = dict(first_block=first, split_endpoints=split)
    got = image.untransform_decode_channel_image(fmt, torch.from_numpy(t.copy()).to(dev), w, h, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(image.untransform_decode_channel_image(fmt, t, w, h, **kw), want)
    got = image.decode_channel_image(fmt, torch.from_numpy(x[first * bs:(first + num) * bs].copy()).to(dev), w, h)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    # a caller's buffer and pitch: the padding stays as it was
    pitch = BPP[fmt] * w + 6
    out = torch.full((pitch * h,), 0xA5, dtype=torch.uint8, device=dev)
    assert image.untransform_decode_channel_image(fmt, torch.from_numpy(t.copy()).to(dev), w, h, out=out, pitch=pitch, **kw) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), expected(oracle, fmt, total, w, h, pitch, first=first))


# ---- case 7: graph capture ---------------------------------------------------------------------------------------------
def test_fused_call_replays_from_a_hip_graph(lib, dev, oracle):
    import torch

    fmt, width, height, split = "bc5", 260, 8, True
    n = blocks_of(width, height)
    pitch = BPP[fmt] * width
    x, t = reference(fmt, n, split)
    src = Guarded(dev, t.size, 0, t)
    dst = Guarded(dev, pitch * height)

    def work():
        rc = lib.dxtlt_untransform_decode_channel_image_device(FMT_ID[fmt], src.ptr, n, 0, width, height, split, dst.ptr, pitch,
                                                               torch.cuda.current_stream(dev).cuda_stream)
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
    for seed in (1, 2):   # new blocks in the same buffer, the output poisoned again: only a replay can produce the right image
        x2, t2 = reference(fmt, n, split, seed=seed)
        assert not np.array_equal(x, x2)
        src.view.copy_(torch.from_numpy(t2.copy()).to(dev))
        dst.view.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert np.array_equal(dst.bytes(), expected(oracle, fmt, n, width, height, pitch, seed=seed))
        assert np.array_equal(src.bytes(), t2)
