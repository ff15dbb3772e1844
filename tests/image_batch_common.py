"""What tests/test_image_batch_layout.py and tests/test_image_batch_gpu.py share (include/dxtlt_image.h, "many buffers in one
call"): the ctypes declarations of dxtlt_untransform_decode_images_batch_device and of its planning hook, and the batches of
the GPU tests as plain data -- so that the layout test can prove on a machine without a GPU, through the hook, which tile forms
and lookup paths those batches reach."""
from __future__ import annotations

import collections
import ctypes as C

from image_regions_common import (BPP, CHAIN_256, CHAIN_260, CUBE, FMTS, FMT_ID, GAPS, TOTAL_256, TOTAL_260, Region, blocks_of,
                                  default_settings, load as load_regions, other_settings, region_end, settings_of)

TILE = {"bc1": 512, "bc2": 256, "bc3": 256, "bc4": 512, "bc5": 256}   # blocks of a 256-lane tile


class BatchItem(C.Structure):   # DxtltImageBatchItem, include/dxtlt_image.h
    _fields_ = [("d_transformed", C.c_void_p), ("total_blocks", C.c_uint64), ("regions", C.POINTER(Region)),
                ("region_count", C.c_uint32), ("format", C.c_uint8), ("decorrelation_mode", C.c_uint8),
                ("split_alpha_endpoints", C.c_uint8), ("split_colour_endpoints", C.c_uint8)]


class PlannedEntry(C.Structure):   # DxtltDebugImageBatchEntry
    _fields_ = [("item", C.c_uint32), ("first_region", C.c_uint32), ("region_count", C.c_uint32), ("launch", C.c_int32),
                ("first_wg", C.c_uint32), ("end_wg", C.c_uint32), ("full_tiles", C.c_uint32), ("form", C.c_uint32),
                ("first_block", C.c_uint64), ("range_blocks", C.c_uint64), ("wide_index", C.c_uint32), ("launch_wgs", C.c_uint32)]


def load(pkg):
    l = load_regions(pkg)
    l.dxtlt_untransform_decode_images_batch_device.argtypes = [C.POINTER(BatchItem), C.c_size_t, C.c_void_p]
    l.dxtlt_untransform_decode_images_batch_device.restype = C.c_int32
    l.dxtlt_debug_plan_image_batch.argtypes = [C.POINTER(BatchItem), C.c_size_t, C.POINTER(PlannedEntry), C.c_size_t]
    l.dxtlt_debug_plan_image_batch.restype = C.c_int32
    l.dxtlt_last_error.restype = C.c_char_p
    return l


# One item of a GPU test's batch.  in_off: the source's address modulo 256; out_offs / pitches: per region, the pixel pointer's
# address modulo 256 and the pitch (default 0 and bpp * width); share: items with the same key read ONE source buffer.
Item = collections.namedtuple("Item", "fmt settings total regions in_off seed pitches out_offs share", defaults=(0, 0, None, None, None))


def item_pitches(it):
    return list(it.pitches) if it.pitches else [BPP[it.fmt] * w for _, w, _ in it.regions]


def item_out_offs(it):
    return list(it.out_offs) if it.out_offs else [0] * len(it.regions)


def batch_items(items, addresses, pointers, keep):
    """the DxtltImageBatchItem array of `items`: addresses[i] the source address, pointers[i][k] region k's pixel pointer;
    `keep` collects the region arrays, which must outlive the call"""
    arr = (BatchItem * max(1, len(items)))()
    for i, it in enumerate(items):
        regs = (Region * max(1, len(it.regions)))()
        for k, (first, w, h) in enumerate(it.regions):
            regs[k] = Region(first, w, h, pointers[i][k], item_pitches(it)[k])
        keep.append(regs)
        arr[i] = BatchItem(addresses[i], it.total, regs, len(it.regions), FMT_ID[it.fmt], it.settings[0], int(it.settings[1]),
                           int(it.settings[2]))
    return arr


def plan(lib, items, addresses=None, pointers=None):
    """the planning hook's records for `items` (None: a batch the call refuses).  Default addresses: what Guarded gives --
    a multiple of 256 plus the item's in_off / the region's out_off"""
    if addresses is None:
        addresses = [0x10000000 + 0x100000 * i + it.in_off for i, it in enumerate(items)]
    if pointers is None:
        pointers = [[0x7000000000 + 0x10000000 * i + 0x100000 * k + off for k, off in enumerate(item_out_offs(it))]
                    for i, it in enumerate(items)]
    keep = []
    arr = batch_items(items, addresses, pointers, keep)
    n = lib.dxtlt_debug_plan_image_batch(arr, len(items), None, 0)
    if n < 0:
        return None
    out = (PlannedEntry * max(1, n))()
    assert lib.dxtlt_debug_plan_image_batch(arr, len(items), out, n) == n
    return [out[i] for i in range(n)]


def reached(entries):
    """which tile forms and lookup paths a planned batch runs through"""
    got = set()
    by_launch = collections.defaultdict(list)
    items_seen = collections.Counter(e.item for e in entries)
    if any(c > 1 for c in items_seen.values()):
        got.add("multi-entry item")
    for e in entries:
        if e.launch < 0:
            got.add("alone")
            continue
        by_launch[e.launch].append(e)
        if e.full_tiles > 0:
            got.add("aligned tiles" if e.form == 1 else "shifted tiles")
        if e.end_wg - e.first_wg > e.full_tiles:
            got.add("edge tiles")
        if e.end_wg - e.first_wg >= 8:
            got.add("rotation")
        if e.wide_index:
            got.add("wide index")
    for es in by_launch.values():
        # the index names the owner of workgroup 64 * (wg / 64); a workgroup of a later entry finds its own by bisection
        for e in es:
            if any(o.first_wg <= 64 * (wg // 64) < o.end_wg and o.first_wg != e.first_wg
                   for wg in (e.first_wg, e.end_wg - 1) for o in es):
                got.add("bisection")
                break
    return got


# ---- the batches of the GPU tests ------------------------------------------------------------------------------------
LEVEL_64 = [(0, 64, 64)]           # level 0 of a 64 x 64 chain of 5 levels: 256 of the buffer's 341 blocks
ONE_PIXEL = [(340, 1, 1)]          # its last level: one block, one pixel
TOTAL_64 = 341


def mixed_batch():
    """all five formats x {default, other} settings x four shapes, shape by shape so that no launch's items are neighbours,
    with an item without regions and an all-empty item in the middle"""
    items = []
    shapes = [(CHAIN_256, TOTAL_256), (CHAIN_260, TOTAL_260), (LEVEL_64, TOTAL_64), (ONE_PIXEL, TOTAL_64)]
    for s, (regions, total) in enumerate(shapes):
        for fmt in FMTS:
            for settings in (default_settings(fmt), other_settings(fmt)):
                items.append(Item(fmt, settings, total, list(regions), seed=s))
        if s == 1:
            items.append(Item("bc2", default_settings("bc2"), TOTAL_64, []))
            items.append(Item("bc5", default_settings("bc5"), TOTAL_64, [(7, 0, 9), (2**63, 5, 0)]))
    return items


def every_setting_batch():
    return [Item(fmt, settings, TOTAL_260, list(CHAIN_260)) for fmt in FMTS for settings in settings_of(fmt)]


ALIGNED_TOTAL = 8192
ALIGNED_REGIONS = [(4096, 128, 128), (5120, 64, 64), (5376, 36, 8)]


def aligned_batch():
    """the shapes of test_regions_whose_stream_bases_are_on_128_byte_lines beside a misaligned item of the same settings"""
    items = []
    for fmt in FMTS:
        settings = default_settings(fmt)
        items.append(Item(fmt, settings, ALIGNED_TOTAL, ALIGNED_REGIONS[:3]))
        items.append(Item(fmt, settings, TOTAL_256, list(CHAIN_256)))
        items.append(Item(fmt, settings, ALIGNED_TOTAL, ALIGNED_REGIONS[:2], seed=1))
    return items


SMALL = [(0, 16, 16)]   # 16 blocks


def many_small_batch():
    """300 items of a 16 x 16 image and three whole chains per format, BC1 and BC4: one launch each"""
    items = []
    for fmt in ("bc1", "bc4"):
        settings = default_settings(fmt)
        for i in range(300):
            if i in (0, 150, 299):
                items.append(Item(fmt, settings, TOTAL_256, list(CHAIN_256), seed=i))
            items.append(Item(fmt, settings, 16, list(SMALL), seed=i))
    return items


def many_regions(count):
    """`count` regions side by side, of 4, 1, 6 and 2 blocks in turn; the total"""
    sizes = [(8, 8), (4, 4), (12, 8), (5, 3)]
    regions, at = [], 0
    for i in range(count):
        w, h = sizes[i % 4]
        regions.append((at, w, h))
        at += blocks_of(w, h)
    return regions, at


def multi_entry_batch():
    items = []
    for fmt in FMTS:
        settings = default_settings(fmt)
        for count in (17, 33):
            regions, total = many_regions(count)
            items.append(Item(fmt, settings, total, regions, seed=count))
        items.append(Item(fmt, settings, 6 * 341, list(CUBE)))
    return items


def gaps_batch():
    return [Item(fmt, default_settings(fmt), TOTAL_256, list(GAPS), pitches=[max(BPP[fmt] * w, 16) for _, w, _ in GAPS]) for fmt in FMTS]


def shared_buffer_batch():
    """two items per format over ONE source: the even and the odd levels of a chain"""
    items = []
    for fmt in FMTS:
        settings = default_settings(fmt)
        items.append(Item(fmt, settings, TOTAL_256, CHAIN_256[0::2], share=fmt))
        items.append(Item(fmt, settings, TOTAL_256, CHAIN_256[1::2], share=fmt))
    return items


def store_policy_batch():
    """pixel pointers at +0, +4 and +8 from a 16-byte boundary and pitches that are and are not multiples of 16, mixed inside
    an item and across items; a BC4 image at an odd address with an odd pitch"""
    items = []
    for fmt in FMTS:
        bpp, settings = BPP[fmt], default_settings(fmt)
        row = [bpp * w for _, w, _ in CHAIN_260]
        pitches, offs = list(row), [0] * len(CHAIN_260)
        pitches[0] = (row[0] + 15) // 16 * 16
        pitches[1] = row[1] + 20
        offs[2], offs[3], offs[4] = 4, 8, 12
        if fmt == "bc4":
            offs[5], pitches[5] = 3, row[5] + 3
        items.append(Item(fmt, settings, TOTAL_260, list(CHAIN_260), pitches=pitches, out_offs=offs))
        # the same chain again with every image at +8 and a pitch that is no multiple of 16, and once more all on 16
        items.append(Item(fmt, settings, TOTAL_260, list(CHAIN_260), seed=1, pitches=[(r + 15) // 16 * 16 + 8 for r in row],
                          out_offs=[8] * len(row)))
        items.append(Item(fmt, settings, TOTAL_260, list(CHAIN_260), seed=2, pitches=[(r + 15) // 16 * 16 for r in row]))
    return items


def fallback_batch():
    """an item whose buffer sits at an odd address between two ordinary ones"""
    items = []
    for fmt in FMTS:
        settings = default_settings(fmt)
        items.append(Item(fmt, settings, TOTAL_260, list(CHAIN_260)))
        items.append(Item(fmt, settings, TOTAL_256, list(CHAIN_256), in_off=1, seed=1))
        items.append(Item(fmt, settings, TOTAL_260, list(CHAIN_260), seed=2))
    return items


GPU_BATCHES = {"mixed": mixed_batch, "every setting": every_setting_batch, "aligned": aligned_batch, "many small": many_small_batch,
               "multi entry": multi_entry_batch, "gaps": gaps_batch, "shared buffer": shared_buffer_batch,
               "store policy": store_policy_batch, "fallback": fallback_batch}
