"""What tests/test_bc6h_image_regions_layout.py and tests/test_bc6h_image_regions_gpu.py share (include/dxtlt_bc6h_image.h, "several
images of one BC6H buffer"): the ctypes declarations.  The plain Python statement of the launch plan and the region lists of the
cases are tests/bc7_image_regions_common.py's and tests/image_regions_common.py's -- block counts and the granule plan do not
depend on the format -- and are passed on from here."""
from __future__ import annotations

import ctypes as C

from bc7_image_regions_common import (E_ARGUMENT, E_LENGTH, FACE_BLOCKS, GRANULE, MAX_GRANULES, OK, THREE_FACES, TOTAL_THREE, TOTAL_TWO,  # noqa: F401
                                      TWO_FACES, groups_of, plan_of)
from bc7_image_regions_common import Launch as Bc7Launch
from image_regions_common import CHAIN_256, PER_LAUNCH, TOTAL_256, Region, blocks_of, region_array, region_end  # noqa: F401

BPP = 8   # RGBA16F


class Launch(C.Structure):   # DxtltBc6hImagesLaunch, include/dxtlt_bc6h_image.h
    _fields_ = [("first_region", C.c_uint32), ("region_count", C.c_uint32), ("first_granule", C.c_uint64),
                ("granule_count", C.c_uint64), ("tail", C.c_uint32), ("reserved", C.c_uint32)]


def load(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, i32, u32, u64, u8, b, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint8, C.c_bool, C.c_size_t
    rp = C.POINTER(Region)
    l.dxtlt_untransform_decode_bc6h_images_device.argtypes = [vp, u64, rp, sz, vp]
    l.dxtlt_decode_bc6h_images_device.argtypes = [vp, u64, rp, sz, vp]
    l.dxtlt_untransform_decode_bc6h_images.argtypes = [vp, sz, rp, sz]
    l.dxtlt_debug_plan_bc6h_images.argtypes = [u64, rp, sz, C.POINTER(Launch), sz]
    l.dxtlt_untransform_decode_bc6h_image_device.argtypes = [vp, u64, u64, u32, u32, vp, u64, vp]
    l.dxtlt_decode_bc6h_image_device.argtypes = [vp, u32, u32, vp, u64, vp]
    l.dxtlt_transform_bc6h.argtypes = [vp, vp, sz]
    l.dxtlt_transform_bc6h_range_device.argtypes = [b, vp, vp, u64, u64, u64, vp]
    l.dxtlt_debug_plan_bc7_images.argtypes = [u64, rp, sz, C.POINTER(Bc7Launch), sz]
    l.dxtlt_untransform_decode_bc7_images_device.argtypes = [vp, u64, rp, sz, vp]
    l.dxtlt_decode_bc7_images_device.argtypes = [vp, u64, rp, sz, vp]
    l.dxtlt_untransform_decode_bc7_images.argtypes = [vp, sz, rp, sz]
    l.dxtlt_untransform_decode_images_device.argtypes = [i32, vp, u64, rp, sz, u8, b, b, vp]
    l.dxtlt_decode_images_device.argtypes = [i32, vp, u64, rp, sz, vp]
    l.dxtlt_untransform_decode_images.argtypes = [i32, vp, sz, rp, sz, u8, b, b]
    for f in (l.dxtlt_untransform_decode_bc6h_images_device, l.dxtlt_decode_bc6h_images_device, l.dxtlt_untransform_decode_bc6h_images,
              l.dxtlt_debug_plan_bc6h_images, l.dxtlt_untransform_decode_bc6h_image_device, l.dxtlt_decode_bc6h_image_device,
              l.dxtlt_transform_bc6h, l.dxtlt_transform_bc6h_range_device, l.dxtlt_debug_plan_bc7_images,
              l.dxtlt_untransform_decode_bc7_images_device, l.dxtlt_decode_bc7_images_device, l.dxtlt_untransform_decode_bc7_images,
              l.dxtlt_untransform_decode_images_device, l.dxtlt_decode_images_device, l.dxtlt_untransform_decode_images):
        f.restype = i32
    l.dxtlt_last_error.restype = C.c_char_p
    return l
