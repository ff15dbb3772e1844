"""What tests/test_bc6h_image_batch_layout.py, tests/test_bc6h_image_batch_defects.py and the BC6H batch GPU tests share
(include/dxtlt_bc6h_image.h, "many buffers in one call"): the ctypes declarations of
dxtlt_untransform_decode_bc6h_images_batch_device and of its planning hook, and the item type of the batches.  The plain Python
statement of the plan is tests/bc7_image_batch_common.py's plan_of -- it does not depend on the format -- and is passed on from
here; regions and the single call's declarations are tests/bc6h_image_regions_common.py's."""
from __future__ import annotations

import collections
import ctypes as C

from bc6h_image_regions_common import BPP, load as load_regions
from bc7_image_batch_common import MAX_WGS, plan_of, shape  # noqa: F401
from image_regions_common import Region


class BatchItem(C.Structure):   # DxtltBc6hImageBatchItem, include/dxtlt_bc6h_image.h
    _fields_ = [("d_transformed", C.c_void_p), ("total_blocks", C.c_uint64), ("regions", C.POINTER(Region)),
                ("region_count", C.c_uint32), ("reserved", C.c_uint32)]


class PlannedEntry(C.Structure):   # DxtltDebugBc6hImageBatchEntry
    _fields_ = [("item", C.c_uint32), ("first_region", C.c_uint32), ("region_count", C.c_uint32), ("tail_index", C.c_int32),
                ("first_granule", C.c_uint64), ("granule_count", C.c_uint32), ("first_wg", C.c_uint32),
                ("granule_wgs", C.c_uint32), ("tail_wgs", C.c_uint32)]


def load(pkg):
    l = load_regions(pkg)
    l.dxtlt_untransform_decode_bc6h_images_batch_device.argtypes = [C.POINTER(BatchItem), C.c_size_t, C.c_void_p]
    l.dxtlt_untransform_decode_bc6h_images_batch_device.restype = C.c_int32
    l.dxtlt_debug_plan_bc6h_image_batch.argtypes = [C.POINTER(BatchItem), C.c_size_t, C.POINTER(PlannedEntry), C.c_size_t]
    l.dxtlt_debug_plan_bc6h_image_batch.restype = C.c_int32
    return l


# One item of a batch.  kind / seed: its data; in_off: the source's address modulo 256; layouts: per region (pitch, the pixel
# pointer's address modulo 256), default (8 * width, 0); share: items with the same key read ONE source buffer.
Item = collections.namedtuple("Item", "total regions kind seed in_off layouts share", defaults=("interleaved", 0, 0, None, None))


def item_layouts(it):
    return list(it.layouts) if it.layouts else [(BPP * w, 0) for _, w, _ in it.regions]


def batch_items(items, addresses, pointers, keep):
    """the DxtltBc6hImageBatchItem array of `items`: addresses[i] the source address, pointers[i][k] region k's pixel pointer;
    `keep` collects the region arrays, which must outlive the call"""
    arr = (BatchItem * max(1, len(items)))()
    for i, it in enumerate(items):
        regs = (Region * max(1, len(it.regions)))()
        for k, ((first, w, h), (pitch, _)) in enumerate(zip(it.regions, item_layouts(it))):
            regs[k] = Region(first, w, h, pointers[i][k], pitch)
        keep.append(regs)
        arr[i] = BatchItem(addresses[i], it.total, regs, len(it.regions), 0)
    return arr


def made_up(items):
    """addresses that are only numbers: a multiple of 256 plus the item's in_off / the region's offset"""
    addresses = [0x10000000 + 0x100000 * i + it.in_off for i, it in enumerate(items)]
    pointers = [[0x7000000000 + 0x10000000 * i + 0x100000 * k + off for k, (_, off) in enumerate(item_layouts(it))]
                for i, it in enumerate(items)]
    return addresses, pointers


def plan(lib, items, addresses=None, pointers=None):
    """the planning hook's records for `items` as shape() tuples (None: a batch the call refuses)"""
    if addresses is None:
        addresses, pointers = made_up(items)
    keep = []
    arr = batch_items(items, addresses, pointers, keep)
    n = lib.dxtlt_debug_plan_bc6h_image_batch(arr, len(items), None, 0)
    if n < 0:
        return None
    out = (PlannedEntry * max(1, n))()
    assert lib.dxtlt_debug_plan_bc6h_image_batch(arr, len(items), out, n) == n
    return [shape(out[i]) for i in range(n)]
