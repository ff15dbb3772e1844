"""What tests/test_bc7_image_regions_layout.py and tests/test_bc7_image_regions_gpu.py share (include/dxtlt_bc7_image.h, "several
images of one BC7 buffer"): the ctypes declarations, the plain Python statement of the launch plan, and the region lists of the
cases.  The region type, the mip-chain statement and the guarded arenas are tests/image_regions_common.py's."""
from __future__ import annotations

import ctypes as C

from image_regions_common import PER_LAUNCH, Region, blocks_of, mip_chain, region_end

OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
GRANULE = 1024
MAX_GRANULES = 1 << 21   # per launch (csrc/granule_sort.h)


class Launch(C.Structure):   # DxtltBc7ImagesLaunch, include/dxtlt_bc7_image.h
    _fields_ = [("first_region", C.c_uint32), ("region_count", C.c_uint32), ("first_granule", C.c_uint64),
                ("granule_count", C.c_uint64), ("tail", C.c_uint32), ("reserved", C.c_uint32)]


def load(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, i32, u32, u64, u8, b, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint8, C.c_bool, C.c_size_t
    rp = C.POINTER(Region)
    l.dxtlt_untransform_decode_bc7_images_device.argtypes = [vp, u64, rp, sz, vp]
    l.dxtlt_decode_bc7_images_device.argtypes = [vp, u64, rp, sz, vp]
    l.dxtlt_untransform_decode_bc7_images.argtypes = [vp, sz, rp, sz]
    l.dxtlt_debug_plan_bc7_images.argtypes = [u64, rp, sz, C.POINTER(Launch), sz]
    l.dxtlt_untransform_decode_bc7_image_device.argtypes = [vp, u64, u64, u32, u32, vp, u64, vp]
    l.dxtlt_decode_bc7_image_device.argtypes = [vp, u32, u32, vp, u64, vp]
    l.dxtlt_transform_bc7.argtypes = [vp, vp, sz]
    l.dxtlt_untransform_decode_images_device.argtypes = [i32, vp, u64, rp, sz, u8, b, b, vp]
    l.dxtlt_decode_images_device.argtypes = [i32, vp, u64, rp, sz, vp]
    l.dxtlt_untransform_decode_images.argtypes = [i32, vp, sz, rp, sz, u8, b, b]
    for f in (l.dxtlt_untransform_decode_bc7_images_device, l.dxtlt_decode_bc7_images_device, l.dxtlt_untransform_decode_bc7_images,
              l.dxtlt_debug_plan_bc7_images, l.dxtlt_untransform_decode_bc7_image_device, l.dxtlt_decode_bc7_image_device,
              l.dxtlt_transform_bc7, l.dxtlt_untransform_decode_images_device, l.dxtlt_decode_images_device,
              l.dxtlt_untransform_decode_images):
        f.restype = i32
    l.dxtlt_last_error.restype = C.c_char_p
    return l


def groups_of(regions):
    """the non-empty regions in groups of at most PER_LAUNCH consecutive ones: [(index of the first, [regions])]"""
    groups, at, now = [], None, []
    for i, r in enumerate(regions):
        if r[1] == 0 or r[2] == 0:
            continue
        if not now:
            at = i
        now.append(r)
        if len(now) == PER_LAUNCH:
            groups.append((at, now))
            now = []
    if now:
        groups.append((at, now))
    return groups


def plan_of(total, regions):
    """the plain Python statement of the plan: [(first region, region count, first granule, granule count, tail)] -- per group
    one launch over the main part's granules its covering range touches, split at 2^21, and the tail launch if it reaches the
    tail part"""
    main = total - total % GRANULE
    out = []
    for at, group in groups_of(regions):
        first, end = group[0][0], region_end(group[-1])
        if first < main:
            g0, g1 = first // GRANULE, (min(end, main) - 1) // GRANULE
            for g in range(g0, g1 + 1, MAX_GRANULES):
                out.append((at, len(group), g, min(MAX_GRANULES, g1 + 1 - g), 0))
        if end > main:
            out.append((at, len(group), main // GRANULE, 1, 1))
    return out


# ---- the region lists of the cases ------------------------------------------------------------------------------------------
FACE, FACE_BLOCKS = mip_chain(128, 128, 8)     # 1024 + 256 + 64 + 16 + 4 + 1 + 1 + 1
assert FACE_BLOCKS == 1367 and [blocks_of(w, h) for _, w, h in FACE] == [1024, 256, 64, 16, 4, 1, 1, 1]


def faces(n):
    """n faces of the 128 x 128 eight-level chain behind one another, and their blocks"""
    return [r for f in range(n) for r in mip_chain(128, 128, 8, FACE_BLOCKS * f)[0]], FACE_BLOCKS * n


TWO_FACES, TOTAL_TWO = faces(2)       # 2734 blocks, main part 2048: sixteen regions, one group
THREE_FACES, TOTAL_THREE = faces(3)   # 4101 blocks, tail part of 5: 24 regions, two groups that share granule 2
assert (TOTAL_TWO, len(TWO_FACES), TOTAL_THREE, len(THREE_FACES)) == (2734, 16, 4101, 24)
assert TWO_FACES[8][0] == 1367 and 1367 % 64 == 23                      # face 1's level 0: mid-granule, lane 23 of a wave
assert TWO_FACES[8][0] < 2048 < region_end(TWO_FACES[8])                # ... and across the main / tail boundary
assert sum(1 for r in TWO_FACES if 1024 < r[0] < 2048) == 7              # seven region boundaries inside main granule 1
