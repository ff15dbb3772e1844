"""BC6H decoders on the MI355X (include/dxtlt_bc6h_image.h): the block decoder, the plain image decoder and the fused untransform
+ decode call against the numpy statement of tests/bc6h_decode_ref.py, byte for byte.  Every output sits inside guard bytes and
is prefilled with 0xA5: the guards, the pitch padding and the pixels a clipped block does not have must still be 0xA5
afterwards, and the source is unchanged.  Transformed buffers come from dxtlt_transform_bc6h.  The largest buffer is 5463
blocks."""
import ctypes as C
import os

import numpy as np
import pytest

import bc6h_decode_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256   # a payload at offset 0 stays on a 256-byte address
OK = 0
GRANULE = 1024
BPP = 8
TOTALS = (1, 37, 1023, 1024, 1025, 2391, 5463)
KINDS = {"balanced": ref.mode_balanced_blocks, "wave_uniform": ref.wave_uniform_blocks, "interleaved": ref.interleaved_class_blocks}


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, i32, u32, u64, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_size_t
    l.dxtlt_decode_bc6h_blocks_device.argtypes = [vp, sz, vp, sz, vp]
    l.dxtlt_decode_bc6h_image_device.argtypes = [vp, u32, u32, vp, u64, vp]
    l.dxtlt_untransform_decode_bc6h_image_device.argtypes = [vp, u64, u64, u32, u32, vp, u64, vp]
    l.dxtlt_untransform_decode_bc6h_image.argtypes = [vp, sz, u64, u32, u32, vp, u64]
    l.dxtlt_transform_bc6h.argtypes = [vp, vp, sz]
    l.dxtlt_transform_bc6h_range_device.argtypes = [C.c_bool, vp, vp, u64, u64, u64, vp]
    l.dxtlt_image_mip_level.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64),
                                        C.POINTER(u64)]
    for f in (l.dxtlt_decode_bc6h_blocks_device, l.dxtlt_decode_bc6h_image_device, l.dxtlt_untransform_decode_bc6h_image_device,
              l.dxtlt_untransform_decode_bc6h_image, l.dxtlt_transform_bc6h, l.dxtlt_transform_bc6h_range_device, l.dxtlt_image_mip_level):
        f.restype = i32
    return l


_cache = {}


def reference(lib, kind, total, seed=0):
    """(blocks (total, 16), their pixels (total, 16, 4) uint16, the transformed buffer) of a whole array, computed once and shared"""
    key = (kind, total, seed)
    if key not in _cache:
        x = KINDS[kind](total, 100 + seed)
        t = np.zeros(x.size, dtype=np.uint8)
        assert lib.dxtlt_transform_bc6h(x.ctypes.data, t.ctypes.data, x.size) == OK
        px = ref.decode_blocks(x)
        for a in (x, t, px):
            a.setflags(write=False)
        _cache[key] = (x, px, t)
    return _cache[key]


def expected_buffer(pixels, width, height, pitch):
    """the pitch * height bytes of an output prefilled with 0xA5 that received the image of the row-major blocks' pixels"""
    out = np.full(pitch * height, 0xA5, dtype=np.uint8)
    out.reshape(height, pitch)[:, :BPP * width] = ref.image_bytes(pixels, width, height)
    return out


class Guarded:
    """`n` device bytes at offset `off` from a 256-byte aligned address, GUARD + off bytes of 0xA5 in front and GUARD behind"""

    def __init__(self, dev, n, off=0, data=None):
        import torch

        self.n, self.at = n, GUARD + off
        self.base = torch.full((self.at + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert self.base.data_ptr() % 256 == 0
        if data is not None:
            self.base[self.at:self.at + n].copy_(torch.from_numpy(np.array(data, copy=True).reshape(-1)).to(dev))
        self.ptr = self.base.data_ptr() + self.at
        self.view = self.base[self.at:self.at + n]

    def bytes(self):
        """the payload, after checking the guards"""
        host = self.base.cpu().numpy()
        assert (host[:self.at] == 0xA5).all() and (host[self.at + self.n:] == 0xA5).all(), "guard bytes were written"
        return host[self.at:self.at + self.n]


def run_fused(lib, dev, transformed, total, first, width, height, pitch=None, out_off=0, in_off=0):
    import torch

    pitch = BPP * width if pitch is None else pitch
    src = Guarded(dev, transformed.size, in_off, transformed)
    dst = Guarded(dev, pitch * height, out_off)
    with torch.cuda.device(dev):
        rc = lib.dxtlt_untransform_decode_bc6h_image_device(src.ptr, total, first, width, height, dst.ptr, pitch,
                                                            torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), transformed), "the transformed buffer changed"
    return dst.bytes()


def run_plain(lib, dev, blocks, width, height, pitch=None, out_off=0, in_off=0):
    import torch

    pitch = BPP * width if pitch is None else pitch
    blocks = np.ascontiguousarray(blocks).reshape(-1)
    src = Guarded(dev, blocks.size, in_off, blocks)
    dst = Guarded(dev, pitch * height, out_off)
    with torch.cuda.device(dev):
        rc = lib.dxtlt_decode_bc6h_image_device(src.ptr, width, height, dst.ptr, pitch, torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), blocks), "the block array changed"
    return dst.bytes()


def blocks_of(width, height):
    return ((width + 3) // 4) * ((height + 3) // 4)


def shape_of(n):
    """an image of exactly n blocks whose last block column and row are clipped: as many block rows (at most 40) as divide n"""
    bh = max(d for d in range(1, 41) if n % d == 0)
    return 4 * (n // bh) - 1, 4 * bh - 2


# ---- blocks -> 128-byte records -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["fixture", "balanced", "interleaved"])
def test_block_decode_at_aligned_and_odd_pointers(lib, dev, source):
    import torch

    if source == "fixture":
        with np.load(os.path.join(ROOT, "tests", "golden", "bc6h_decode_vectors.npz")) as z:
            x = z["blocks"]
    else:
        x = KINDS[source](4096, 5)
    want = ref.records(ref.decode_blocks(x))
    for in_off in (0, 1):
        for out_off in (0, 8, 4):   # 16-byte stores on a 16-byte and on an 8-byte address, byte stores
            src = Guarded(dev, x.size, in_off, x)
            dst = Guarded(dev, want.size, out_off)
            with torch.cuda.device(dev):
                assert lib.dxtlt_decode_bc6h_blocks_device(src.ptr, x.size, dst.ptr, want.size, torch.cuda.current_stream().cuda_stream) == OK
            torch.cuda.synchronize()
            assert np.array_equal(dst.bytes().reshape(-1, 128), want), (in_off, out_off)
            assert np.array_equal(src.bytes(), x.reshape(-1))


# ---- blocks in block order -> image -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (4, 4), (7, 5), (64, 64), (260, 36), (520, 8)])
@pytest.mark.parametrize("kind", list(KINDS))
def test_plain_image_every_shape_pitch_and_pointer(lib, dev, kind, shape):
    width, height = shape
    n = blocks_of(width, height)
    x = KINDS[kind](n, 6)
    px = ref.decode_blocks(x)
    for pitch in (BPP * width, BPP * width + 16, BPP * width + 8):
        want = expected_buffer(px, width, height, pitch)
        for out_off in (0, 8):      # pointer and pitch multiples of 16, and of 8 only
            for in_off in (0, 8):   # vector loads, byte loads
                got = run_plain(lib, dev, x, width, height, pitch, out_off, in_off)
                assert np.array_equal(got, want), (pitch, out_off, in_off)


# ---- fused ------------------------------------------------------------------------------------------------------------------
def ranges_of(total):
    """(name, first_block, blocks) of the ranges this total has"""
    main = total - total % GRANULE
    tail = total - main
    out = [("whole", 0, total), ("first block", 0, 1), ("last block", total - 1, 1)]
    if main >= GRANULE:
        out.append(("inside one granule", 100, 300))
    elif total >= 30:
        out.append(("inside the tail part", 5, 20))
    if main >= 3 * GRANULE:
        out.append(("mid-granule over three granules", 700, 2000))
    if main >= 2 * GRANULE and tail >= 2:
        out.append(("mid-granule into the tail part", 700, main + tail // 2 - 700))
    if main >= GRANULE and tail >= 2:
        out.append(("ends inside the tail part", main - 300, 300 + tail // 2))
    if main >= GRANULE and tail >= 8:
        out.append(("wholly inside the tail part", main + 3, tail - 5))
    return out


def test_the_totals_have_every_kind_of_range():
    names = {name for total in TOTALS for name, _, _ in ranges_of(total)}
    assert names == {"whole", "first block", "last block", "inside one granule", "inside the tail part",
                     "mid-granule over three granules", "mid-granule into the tail part", "ends inside the tail part",
                     "wholly inside the tail part"}
    assert all(0 <= first and first + n <= total and n > 0 for total in TOTALS for _, first, n in ranges_of(total))


@pytest.mark.parametrize("total", TOTALS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_ranges(lib, dev, kind, total):
    x, px, t = reference(lib, kind, total)
    for name, first, n in ranges_of(total):
        width, height = shape_of(n)
        assert blocks_of(width, height) == n
        # an aligned pitch and pointer (streaming stores) and an odd pair (plain stores), the padding checked in both
        aligned_pitch = (BPP * width + 15) // 16 * 16 + 16
        for pitch, out_off in ((aligned_pitch, 0), (BPP * width + 8, 8)):
            want = expected_buffer(px[first:first + n], width, height, pitch)
            got = run_fused(lib, dev, t, total, first, width, height, pitch, out_off)
            assert np.array_equal(got, want), (name, first, n, pitch, out_off)
            if name in ("whole", "mid-granule over three granules", "ends inside the tail part"):
                plain = run_plain(lib, dev, x[first:first + n], width, height, pitch, out_off)
                assert np.array_equal(plain, got), ("plain", name)


@pytest.mark.parametrize("cls", range(ref.CLASSES))
def test_fused_on_a_buffer_of_one_class(lib, dev, cls):
    total = 1300   # a granule and a tail part
    x = ref.single_class_blocks(total, cls, 40 + cls)
    t = np.zeros(x.size, dtype=np.uint8)
    assert lib.dxtlt_transform_bc6h(x.ctypes.data, t.ctypes.data, x.size) == OK
    width, height = shape_of(total)
    want = expected_buffer(ref.decode_blocks(x), width, height, BPP * width)
    assert np.array_equal(run_fused(lib, dev, t, total, 0, width, height), want)


def test_fused_with_an_unaligned_transformed_buffer(lib, dev):
    """dxtlt_transform_bc6h_range_device accepts any address: the transformed buffer is made on the device at one that is no
    multiple of 16, and decoded from there"""
    import torch

    total = 2391
    x, px, t = reference(lib, "balanced", total)
    width, height = shape_of(total)
    want = expected_buffer(px, width, height, BPP * width)
    for in_off in (1, 8):
        src = Guarded(dev, x.size, 0, x)
        mid = Guarded(dev, x.size, in_off)
        dst = Guarded(dev, want.size)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            assert lib.dxtlt_transform_bc6h_range_device(False, src.ptr, mid.ptr, total, 0, total, stream) == OK
            assert lib.dxtlt_untransform_decode_bc6h_image_device(mid.ptr, total, 0, width, height, dst.ptr, BPP * width, stream) == OK
        torch.cuda.synchronize()
        assert np.array_equal(mid.bytes(), t), in_off
        assert np.array_equal(dst.bytes(), want), in_off


def mip_level(lib, width, height, mip_count, level):
    w, h = C.c_uint32(), C.c_uint32()
    first, num, total = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.dxtlt_image_mip_level(width, height, mip_count, level, C.byref(w), C.byref(h), C.byref(first), C.byref(num),
                                     C.byref(total)) == OK
    return w.value, h.value, first.value, num.value, total.value


def test_every_level_of_a_transformed_mip_chain(lib, dev):
    levels = [mip_level(lib, 256, 256, 9, k) for k in range(9)]
    total = levels[0][4]
    assert total == 5463 and [l[3] for l in levels] == [4096, 1024, 256, 64, 16, 4, 1, 1, 1]
    x, px, t = reference(lib, "balanced", total)
    for k, (w, h, first, num, _) in enumerate(levels):
        want = expected_buffer(px[first:first + num], w, h, BPP * w)
        assert np.array_equal(run_fused(lib, dev, t, total, first, w, h), want), k


def test_host_call_on_two_ranges(lib):
    total = 5463
    x, px, t = reference(lib, "balanced", total)
    for first, n in ((700, 2000), (5120 - 300, 300 + 171)):
        width, height = shape_of(n)
        pitch = BPP * width + 24
        host = np.full(GUARD + pitch * height + GUARD, 0xA5, dtype=np.uint8)
        rc = lib.dxtlt_untransform_decode_bc6h_image(t.ctypes.data, t.size, first, width, height, host.ctypes.data + GUARD, pitch)
        assert rc == OK
        assert (host[:GUARD] == 0xA5).all() and (host[GUARD + pitch * height:] == 0xA5).all()
        assert np.array_equal(host[GUARD:GUARD + pitch * height], expected_buffer(px[first:first + n], width, height, pitch)), first


def test_python_module_on_tensors_and_host_buffers(pkg, lib, dev):
    import torch

    from dxt_lossless_transform_amd import decode, image

    total, first, n = 2391, 700, 1500
    x, px, t = reference(lib, "balanced", total)
    width, height = shape_of(n)
    want = expected_buffer(px[first:first + n], width, height, BPP * width)
    got = image.untransform_decode_bc6h_image(torch.from_numpy(t.copy()).to(dev), width, height, first_block=first)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    # the documented view: (height, width, 4) half floats
    halves = got.view(torch.float16).reshape(height, width, 4).cpu().numpy().view(np.uint16)
    assert np.array_equal(halves, ref.image_of(px[first:first + n], width, height))
    assert np.array_equal(image.untransform_decode_bc6h_image(t, width, height, first_block=first), want)
    got = image.decode_bc6h_image(torch.from_numpy(x[first:first + n].copy().reshape(-1)).to(dev), width, height)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    out = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
    decode.decode_bc6h_blocks(torch.from_numpy(x[first:first + n].copy().reshape(-1)).to(dev), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(-1, 128), ref.records(px[first:first + n]))


def test_fused_call_replays_from_a_hip_graph(lib, dev):
    import torch

    total, first, n = 2391, 700, 1500   # two granules and the tail part: two launches, one behind the other
    width, height = shape_of(n)
    pitch = (BPP * width + 15) // 16 * 16
    x, px, t = reference(lib, "balanced", total)
    src = Guarded(dev, t.size, 0, t)
    dst = Guarded(dev, pitch * height)

    def work():
        rc = lib.dxtlt_untransform_decode_bc6h_image_device(src.ptr, total, first, width, height, dst.ptr, pitch,
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
    # new blocks in the same buffer, the output poisoned again: only a replay can produce the right image
    x2, px2, t2 = reference(lib, "interleaved", total, seed=1)
    assert not np.array_equal(x, x2)
    src.view.copy_(torch.from_numpy(t2.copy()).to(dev))
    dst.view.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(dst.bytes(), expected_buffer(px2[first:first + n], width, height, pitch))
    assert np.array_equal(src.bytes(), t2)
