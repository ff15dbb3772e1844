"""What tests/test_image_regions_layout.py and tests/test_image_regions_gpu.py share (include/dxtlt_image.h, "several images of
one buffer"): the ctypes declarations, the mip-chain statement, the region tables of the issue, and -- as tests/test_image_gpu.py
and tests/test_channel_image_gpu.py build theirs -- seeded blocks, the oracle's transform for the input and the oracle's decoder
rearranged into rows for the expected images, for all five formats."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import bc45_ref
import channel_image_ref

OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
FMTS = ("bc1", "bc2", "bc3", "bc4", "bc5")
FMT_ID = {"bc1": 1, "bc2": 2, "bc3": 3, "bc4": 4, "bc5": 5}
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16, "bc4": 8, "bc5": 16}
BPP = {"bc1": 4, "bc2": 4, "bc3": 4, "bc4": 1, "bc5": 2}
PER_LAUNCH = 16
GUARD = 256


class Region(C.Structure):   # DxtltImageRegion, include/dxtlt_image.h
    _fields_ = [("first_block", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("pixels", C.c_void_p),
                ("pitch", C.c_uint64)]


class PlannedLaunch(C.Structure):   # DxtltDebugPlannedLaunch, include/dxtlt_gfx950.h
    _fields_ = [("kind", C.c_int32), ("threads", C.c_int32), ("workgroups", C.c_uint32), ("full_tiles", C.c_uint32),
                ("range_blocks", C.c_uint64), ("aos_offset", C.c_uint64), ("shift", C.c_uint8 * 6), ("halo_vecs", C.c_uint8),
                ("natural", C.c_uint8), ("gbase", C.c_uint64 * 6)]


def load(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, i32, u32, u64, u8, b, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint8, C.c_bool, C.c_size_t
    rp = C.POINTER(Region)
    l.dxtlt_untransform_decode_images_device.argtypes = [i32, vp, u64, rp, sz, u8, b, b, vp]
    l.dxtlt_decode_images_device.argtypes = [i32, vp, u64, rp, sz, vp]
    l.dxtlt_untransform_decode_images.argtypes = [i32, vp, sz, rp, sz, u8, b, b]
    l.dxtlt_image_mip_chain.argtypes = [u32, u32, u32, u64, rp, C.POINTER(u64)]
    l.dxtlt_image_mip_level.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64),
                                        C.POINTER(u64)]
    l.dxtlt_untransform_decode_image_device.argtypes = [i32, vp, u64, u64, u32, u32, u8, b, b, vp, u64, vp]
    l.dxtlt_untransform_decode_channel_image_device.argtypes = [i32, vp, u64, u64, u32, u32, b, vp, u64, vp]
    l.dxtlt_debug_plan_transform.argtypes = [i32, i32, i32, i32, i32, u64, u64, u64, u64, u64, C.POINTER(PlannedLaunch), i32]
    for f in (l.dxtlt_untransform_decode_images_device, l.dxtlt_decode_images_device, l.dxtlt_untransform_decode_images,
              l.dxtlt_image_mip_chain, l.dxtlt_image_mip_level, l.dxtlt_untransform_decode_image_device,
              l.dxtlt_untransform_decode_channel_image_device, l.dxtlt_debug_plan_transform):
        f.restype = i32
    return l


def blocks_of(width, height):
    return ((width + 3) // 4) * ((height + 3) // 4)


def mip_chain(width, height, mip_count, first=0):
    """the Python statement: ([(first block, level width, level height)], the block just behind the chain)"""
    levels = []
    for k in range(mip_count):
        w, h = max(1, width >> k), max(1, height >> k)
        levels.append((first, w, h))
        first += blocks_of(w, h)
    return levels, first


def region_end(region):
    return region[0] + blocks_of(region[1], region[2])


# ---- the tables of the issue ---------------------------------------------------------------------------------------------
CHAIN_256, TOTAL_256 = mip_chain(256, 256, 9)          # 5463 blocks
CHAIN_260, TOTAL_260 = mip_chain(260, 136, 9)          # 2210, 561, 153, 40, 8, 2, 1, 1, 1 = 2977 blocks, clipped blocks at most levels
assert TOTAL_256 == 5463 and TOTAL_260 == 2977
assert [blocks_of(w, h) for _, w, h in CHAIN_260] == [2210, 561, 153, 40, 8, 2, 1, 1, 1]
# levels 0, 2 and 5 of the 256 x 256 chain with a zero-width region between them
GAPS = [CHAIN_256[0], (2**63, 0, 7), CHAIN_256[2], (5400, 0, 0), CHAIN_256[5]]
# six faces of a 64 x 64 chain of 5 levels, 341 blocks each
CUBE = [r for face in range(6) for r in mip_chain(64, 64, 5, 341 * face)[0]]
assert len(CUBE) == 30 and region_end(CUBE[-1]) == 6 * 341


def settings_of(fmt):
    """every setting of the format as (decorrelation mode, split alpha / split_endpoints, split colour): 8 / 8 / 16 / 2 / 2"""
    if fmt in ("bc4", "bc5"):
        return [(0, False, False), (0, True, False)]
    return [(v, sa, sc) for v in range(4) for sa in ((False, True) if fmt == "bc3" else (False,)) for sc in (False, True)]


def default_settings(fmt):
    return (0, True, False) if fmt in ("bc4", "bc5") else (1, True, True)


def other_settings(fmt):
    return {"bc1": (3, False, False), "bc2": (3, False, False), "bc3": (2, True, False), "bc4": (0, False, False),
            "bc5": (0, False, False)}[fmt]


def planned_kinds(lib, fmt, settings, address, total, first, num):
    """the tile kinds the inverse direction takes for a range at this transformed-side address (0 aligned, 2 shifted / edge)"""
    out = (PlannedLaunch * 8)()
    n = lib.dxtlt_debug_plan_transform(FMT_ID[fmt], 1, settings[0], int(settings[1]), int(settings[2]), address, 0, total, first, num,
                                       out, 8)
    assert 0 < n <= 8
    return [out[i].kind for i in range(n)]


# ---- inputs and expected images ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_blocks(fmt, n, seed=0):
    """seeded random blocks.  BC4 / BC5: channel_image_ref's.  BC1 - BC3 as in tests/test_image_gpu.py: every 7th block with colour
    endpoints c0 <= c1 (every 21st c0 == c1) -- BC1's three-colour mode and equal endpoints; BC3 alpha endpoints are a0 <= a1 in
    half of the blocks, a0 == a1 in every 35th"""
    if fmt in ("bc4", "bc5"):
        return channel_image_ref.random_blocks(fmt, n, seed)
    bs = BLOCK[fmt]
    x = np.random.default_rng(0x5E61 + 131 * n + FMT_ID[fmt] + 7919 * seed).integers(0, 256, n * bs, dtype=np.uint8).reshape(n, bs)
    at = 0 if fmt == "bc1" else 8
    c = x[:, at:at + 4].copy().view("<u2")
    lo, hi = c.min(axis=1), c.max(axis=1)
    c[::7, 0], c[::7, 1] = lo[::7], hi[::7]
    c[::21, 1] = c[::21, 0]
    x[:, at:at + 4] = c.view(np.uint8)
    if fmt == "bc3":
        x[::35, 1] = x[::35, 0]
    x.setflags(write=False)
    return x.reshape(-1)


_transformed = {}


def reference(oracle, fmt, n, settings, seed=0):
    """(blocks, transformed) of a whole array of n blocks, computed once per case and shared; neither is writable"""
    key = (fmt, n, settings, seed)
    if key not in _transformed:
        x = random_blocks(fmt, n, seed)
        if fmt in ("bc4", "bc5"):
            t = bc45_ref.transform(fmt, x, settings[1])
        else:
            t = oracle.transform(fmt, x, settings[0], settings[2], settings[1])
        t.setflags(write=False)
        _transformed[key] = (x, t)
    return _transformed[key]


_images = {}


def image_of(oracle, fmt, n, region, seed=0):
    """the expected height x width x bpp image of a region of random_blocks(fmt, n, seed), computed once and shared"""
    key = (fmt, n, region, seed)
    if key not in _images:
        first, width, height = region
        x = random_blocks(fmt, n, seed)[first * BLOCK[fmt]:region_end(region) * BLOCK[fmt]]
        if fmt in ("bc4", "bc5"):
            img = channel_image_ref.image_of(oracle, fmt, x, width, height)
        else:
            bx, by = (width + 3) // 4, (height + 3) // 4
            px = oracle.decode_blocks(fmt, x).reshape(by, bx, 4, 4, 4)   # block row, block column, pixel row, pixel column, rgba
            img = np.ascontiguousarray(px.transpose(0, 2, 1, 3, 4).reshape(4 * by, 4 * bx, 4)[:height, :width])
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def expected_buffer(image, pitch):
    """pitch * height bytes: the image's rows, 0xA5 everywhere else"""
    return channel_image_ref.expected_buffer(image, pitch)


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


def region_array(regions, pointers, pitches):
    arr = (Region * max(1, len(regions)))()
    for i, (first, width, height) in enumerate(regions):
        arr[i] = Region(first, width, height, pointers[i], pitches[i])
    return arr
