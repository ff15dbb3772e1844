"""The argument behaviour of every image entry point as a table: image_call_defects.json holds, per call, format and batch
item, and per answer ("return code: dxtlt_last_error text"), the cases that give it -- each defect of each call alone, every pair of defects, which pins the
documented order of the checks, and the calls that have nothing to do.  tests/test_image_call_defects.py replays the table
against the built library; the file was recorded before the host side of the image calls was gathered into csrc/image_host.h and
is the statement of "nothing changed".  Regenerate it (python tests/golden/make_image_call_defects.py) only when a check is changed on purpose.

Addresses are made-up numbers.  Every case either has nothing to do (an empty image, no non-empty region, an empty batch) or
carries at least one defect, so no call gets as far as a device or dereferences anything -- also on a machine that has a GPU.
run() checks that: a case with a defect must not return DXTLT_OK, and no case may return a device status."""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "image_call_defects.json")
SRC, DST = 0x7F1000000000, 0x7F2000000000   # made up
U64 = 2**64

vp, i32, u32, u64, u8, b, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint8, C.c_bool, C.c_size_t


class Region(C.Structure):   # DxtltImageRegion, include/dxtlt_image.h
    _fields_ = [("first_block", u64), ("width", u32), ("height", u32), ("pixels", vp), ("pitch", u64)]


class BatchItem(C.Structure):   # DxtltImageBatchItem, include/dxtlt_image.h
    _fields_ = [("d_transformed", vp), ("total_blocks", u64), ("regions", C.POINTER(Region)), ("region_count", u32), ("format", u8),
                ("decorrelation_mode", u8), ("split_alpha_endpoints", u8), ("split_colour_endpoints", u8)]


class Bc7BatchItem(C.Structure):   # DxtltBc7ImageBatchItem, include/dxtlt_bc7_image.h
    _fields_ = [("d_transformed", vp), ("total_blocks", u64), ("regions", C.POINTER(Region)), ("region_count", u32), ("reserved", u32)]


rp = C.POINTER(Region)
SIGNATURES = {
    "dxtlt_decode_image_device": [i32, vp, u32, u32, vp, u64, vp],
    "dxtlt_untransform_decode_image_device": [i32, vp, u64, u64, u32, u32, u8, b, b, vp, u64, vp],
    "dxtlt_untransform_decode_image": [i32, vp, sz, u64, u32, u32, u8, b, b, vp, u64],
    "dxtlt_decode_channel_image_device": [i32, vp, u32, u32, vp, u64, vp],
    "dxtlt_untransform_decode_channel_image_device": [i32, vp, u64, u64, u32, u32, b, vp, u64, vp],
    "dxtlt_untransform_decode_channel_image": [i32, vp, sz, u64, u32, u32, b, vp, u64],
    "dxtlt_image_mip_level": [u32, u32, u32, u32, vp, vp, vp, vp, vp],
    "dxtlt_image_mip_chain": [u32, u32, u32, u64, vp, vp],
    "dxtlt_untransform_decode_images_device": [i32, vp, u64, rp, sz, u8, b, b, vp],
    "dxtlt_decode_images_device": [i32, vp, u64, rp, sz, vp],
    "dxtlt_untransform_decode_images": [i32, vp, sz, rp, sz, u8, b, b],
    "dxtlt_decode_bc7_blocks": [vp, sz, vp, sz],
    "dxtlt_decode_bc7_blocks_device": [vp, sz, vp, sz, vp],
    "dxtlt_decode_bc7_image_device": [vp, u32, u32, vp, u64, vp],
    "dxtlt_untransform_decode_bc7_image_device": [vp, u64, u64, u32, u32, vp, u64, vp],
    "dxtlt_untransform_decode_bc7_image": [vp, sz, u64, u32, u32, vp, u64],
    "dxtlt_untransform_decode_bc7_images_device": [vp, u64, rp, sz, vp],
    "dxtlt_decode_bc7_images_device": [vp, u64, rp, sz, vp],
    "dxtlt_untransform_decode_bc7_images": [vp, sz, rp, sz],
    "dxtlt_debug_plan_bc7_images": [u64, rp, sz, vp, sz],
    "dxtlt_decode_bc6h_blocks": [vp, sz, vp, sz],
    "dxtlt_decode_bc6h_blocks_device": [vp, sz, vp, sz, vp],
    "dxtlt_decode_bc6h_image_device": [vp, u32, u32, vp, u64, vp],
    "dxtlt_untransform_decode_bc6h_image_device": [vp, u64, u64, u32, u32, vp, u64, vp],
    "dxtlt_untransform_decode_bc6h_image": [vp, sz, u64, u32, u32, vp, u64],
    "dxtlt_untransform_decode_bc6h_images_device": [vp, u64, rp, sz, vp],
    "dxtlt_decode_bc6h_images_device": [vp, u64, rp, sz, vp],
    "dxtlt_untransform_decode_bc6h_images": [vp, sz, rp, sz],
    "dxtlt_debug_plan_bc6h_images": [u64, rp, sz, vp, sz],
    "dxtlt_untransform_decode_images_batch_device": [C.POINTER(BatchItem), sz, vp],
    "dxtlt_debug_plan_image_batch": [C.POINTER(BatchItem), sz, vp, sz],
    "dxtlt_untransform_decode_bc7_images_batch_device": [C.POINTER(Bc7BatchItem), sz, vp],
    "dxtlt_debug_plan_bc7_image_batch": [C.POINTER(Bc7BatchItem), sz, vp, sz],
}


def load(path):
    lib = C.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        f = getattr(lib, name)
        f.argtypes, f.restype = argtypes, i32
    lib.dxtlt_last_error.restype = C.c_char_p
    return lib


# ---- one image per call ------------------------------------------------------------------------------------------------------
# family: the calls, their formats (None: the call has no format argument), bytes per pixel, the multiple required of pitch and
# pointer, the block size, whether the fused calls take a decorrelation mode
FAMILIES = [
    dict(calls=("dxtlt_decode_image_device", "dxtlt_untransform_decode_image_device", "dxtlt_untransform_decode_image"),
         fmts=(1, 3), bad_fmts=(0, 4, 5, 6, 7, -1), bpp=lambda f: 4, mult=lambda f: 4, bs=lambda f: 8 if f == 1 else 16, settings="rgba"),
    dict(calls=("dxtlt_decode_channel_image_device", "dxtlt_untransform_decode_channel_image_device",
                "dxtlt_untransform_decode_channel_image"),
         fmts=(4, 5), bad_fmts=(0, 1, 3, 6, -1), bpp=lambda f: f - 3, mult=lambda f: f - 3, bs=lambda f: 8 if f == 4 else 16,
         settings="channel"),
    dict(calls=("dxtlt_decode_bc7_image_device", "dxtlt_untransform_decode_bc7_image_device", "dxtlt_untransform_decode_bc7_image"),
         fmts=(None,), bad_fmts=(), bpp=lambda f: 4, mult=lambda f: 4, bs=lambda f: 16, settings=None),
    dict(calls=("dxtlt_decode_bc6h_image_device", "dxtlt_untransform_decode_bc6h_image_device", "dxtlt_untransform_decode_bc6h_image"),
         fmts=(None,), bad_fmts=(), bpp=lambda f: 8, mult=lambda f: 8, bs=lambda f: 16, settings=None),
]
KINDS = ("plain", "fused", "host")   # the block decoder on device pointers, the fused call on device pointers, on host pointers


def image_defects(fam, fmt, kind):
    """the defects of a single-image call in the documented order of its checks: name -> what it does to the arguments"""
    bpp, mult = fam["bpp"](fmt), fam["mult"](fmt)
    d = {}
    if fmt is not None:
        d["format"] = lambda s: s.update(fmt=0)
    d["null"] = lambda s: s.update(src=None)
    d["small pitch"] = lambda s: s.update(pitch=bpp * s["w"] - mult)
    if mult > 1:
        d["multiple"] = lambda s: s.update(dst=s["dst"] + mult // 2)
    if fam["settings"] == "rgba" and kind != "plain":
        d["mode"] = lambda s: s.update(mode=4)
    if kind != "plain":
        d["range"] = lambda s: s.update(total=3)
    if kind == "host":
        d["len"] = lambda s: s.update(extra=3)
    return d


def image_variants(fam, fmt, kind):
    """other forms of the same defects, each alone"""
    bpp, mult = fam["bpp"](fmt), fam["mult"](fmt)
    v = {"null pixels": lambda s: s.update(dst=None), "null both": lambda s: s.update(src=None, dst=None),
         "small pitch of a wide row": lambda s: s.update(w=0xFFFFFFFF, h=1, pitch=bpp * 0xFFFFFFFF - mult),
         "pitch zero": lambda s: s.update(pitch=0)}
    if mult > 1:
        v["multiple of the pitch"] = lambda s: s.update(pitch=s["pitch"] + mult // 2)
        v["odd pointer"] = lambda s: s.update(dst=s["dst"] + 1)
    if kind != "plain":
        v["first past the end"] = lambda s: s.update(first=101)
        v["end past the end"] = lambda s: s.update(first=97)
        v["first wraps"] = lambda s: s.update(first=U64 - 2)
        v["no blocks at all"] = lambda s: s.update(total=0)
        v["odd source gets as far as the range"] = lambda s: s.update(src=s["src"] + 1, total=3)
        if fam["settings"] == "rgba":
            v["mode 255"] = lambda s: s.update(mode=255)
    if kind == "host":
        v["len one more"] = lambda s: s.update(extra=1)
        v["len one block short and odd"] = lambda s: s.update(total=3, extra=fam["bs"](fmt) - 1)
    for bad in fam["bad_fmts"]:
        v[f"format {bad}"] = lambda s, bad=bad: s.update(fmt=bad)
        v[f"format {bad} and an empty image"] = lambda s, bad=bad: s.update(fmt=bad, w=0)
    return v


def image_args(fam, kind, s):
    head = [] if s["fmt"] is None else [s["fmt"]]
    settings = {"rgba": [s["mode"], True, False], "channel": [True], None: []}[fam["settings"]]
    if kind == "plain":
        return head + [s["src"], s["w"], s["h"], s["dst"], s["pitch"], None]
    if kind == "fused":
        return head + [s["src"], s["total"], s["first"], s["w"], s["h"]] + settings + [s["dst"], s["pitch"], None]
    bs = fam["bs"](s["fmt"]) if s["fmt"] in fam["fmts"] else 16
    return head + [s["src"], s["total"] * bs + s["extra"], s["first"], s["w"], s["h"]] + settings + [s["dst"], s["pitch"]]


def image_cases():
    for fam in FAMILIES:
        for fmt, (kind, call) in itertools.product(fam["fmts"], zip(KINDS, fam["calls"])):
            def base():   # an 8 x 8 image, 4 blocks of 100
                return dict(fmt=fmt, src=SRC, dst=DST, w=8, h=8, pitch=fam["bpp"](fmt) * 8, total=100, first=0, mode=1, extra=0)

            tag = "" if fmt is None else f"format {fmt}: "
            # nothing to do, whatever else is passed
            for name, change in (("zero width", dict(w=0)), ("zero height", dict(h=0))):
                s = base()
                s.update(src=None, dst=None, pitch=1, total=0, first=U64 - 2, mode=9, extra=5)
                s.update(change)
                yield call, tag + "nothing to do, " + name, image_args(fam, kind, s), True
            defects = image_defects(fam, fmt, kind)
            sets = [(n,) for n in defects] + list(itertools.combinations(defects, 2)) + [tuple(defects)]
            for names in sets:
                s = base()
                for n in names:
                    defects[n](s)
                yield call, tag + " + ".join(names), image_args(fam, kind, s), False
            for name, change in image_variants(fam, fmt, kind).items():
                s = base()
                change(s)
                yield call, tag + name, image_args(fam, kind, s), False


# ---- several images of one buffer, and many buffers -------------------------------------------------------------------------------
REGION_CALLS = [   # call, kind, formats (None: no format argument), has a mode, bytes per pixel of a call without a format
    ("dxtlt_decode_images_device", "plain", (1, 3, 4, 5), False, 4),
    ("dxtlt_untransform_decode_images_device", "fused", (1, 3, 4, 5), True, 4),
    ("dxtlt_untransform_decode_images", "host", (1, 3, 4, 5), True, 4),
    ("dxtlt_decode_bc7_images_device", "plain", (None,), False, 4),
    ("dxtlt_untransform_decode_bc7_images_device", "fused", (None,), False, 4),
    ("dxtlt_untransform_decode_bc7_images", "host", (None,), False, 4),
    ("dxtlt_debug_plan_bc7_images", "plan", (None,), False, 4),
    ("dxtlt_decode_bc6h_images_device", "plain", (None,), False, 8),
    ("dxtlt_untransform_decode_bc6h_images_device", "fused", (None,), False, 8),
    ("dxtlt_untransform_decode_bc6h_images", "host", (None,), False, 8),
    ("dxtlt_debug_plan_bc6h_images", "plan", (None,), False, 8),
]


def bpp_of(fmt, px=4):
    """bytes per pixel and the multiple required of pitch and pointer; px: the bytes per pixel of a call without a format"""
    if fmt is None:
        return px, px
    return (4, 4) if fmt <= 3 else (fmt - 3, fmt - 3)


def region_defects(fmt, kind, has_mode, px=4):
    """the defects of a region list in the documented order; regions are [first_block, width, height, pixels, pitch]"""
    bpp, mult = bpp_of(fmt, px)
    d = {}
    if fmt is not None:
        d["format"] = lambda s: s.update(fmt=0)
    d["regions"] = lambda s: s.update(regs=None)
    if kind != "plan":
        d["buffer"] = lambda s: s.update(buf=None)
    d["pixels"] = lambda s: s["regs"][0].__setitem__(3, None)
    d["small pitch"] = lambda s: s["regs"][0].__setitem__(4, bpp * 8 - mult)
    if mult > 1:
        d["multiple"] = lambda s: s["regs"][0].__setitem__(3, (s["regs"][0][3] or 0) + mult // 2)
    d["range"] = lambda s: s["regs"][0].__setitem__(0, 98)
    d["order"] = lambda s: s["regs"][1].__setitem__(0, 2)
    if has_mode and fmt <= 3:
        d["mode"] = lambda s: s.update(mode=4)
    if kind == "host":
        d["len"] = lambda s: s.update(extra=3)
    return d


def region_variants(fmt, kind, has_mode, px=4):
    bpp, mult = bpp_of(fmt, px)

    def set_region(k, i, value):
        return lambda s: s["regs"][k].__setitem__(i, value)

    def both(*changes):
        return lambda s: [c(s) for c in changes]

    v = {"first wraps": set_region(0, 0, U64 - 2), "first past the end": set_region(0, 0, 101),
         "unordered": both(set_region(0, 0, 4), set_region(1, 0, 0)), "pixels of the second region": set_region(1, 3, None),
         "range of the first, pixels of the second region": both(set_region(0, 0, 98), set_region(1, 3, None)),
         "small pitch and order of the second region": both(set_region(1, 4, bpp * 8 - mult), set_region(1, 0, 2)),
         "order across an empty region": lambda s: (s["regs"].insert(1, [2**63, 0, 7, None, 1]), s["regs"][2].__setitem__(0, 2)),
         "no blocks at all": lambda s: s.update(total=0)}
    if mult > 1:
        v["multiple of the pitch"] = set_region(0, 4, bpp * 8 + mult // 2)
    if has_mode and fmt <= 3:
        v["mode 255"] = lambda s: s.update(mode=255)
    if kind == "host":
        v["len one more"] = lambda s: s.update(extra=1)
    if fmt is not None:
        for bad in (0, 6, 7, -1):
            v[f"format {bad}"] = lambda s, bad=bad: s.update(fmt=bad)
            v[f"format {bad} and no regions"] = lambda s, bad=bad: s.update(fmt=bad, regs=None, count=0)
    return v


def region_nothing():
    """lists with nothing to do, whatever else is passed"""
    return {"nothing to do, no regions": lambda s: s.update(regs=None, count=0, buf=None, mode=9, extra=5),
            "nothing to do, empty regions only": lambda s: s.update(regs=[[2**63, 0, 7, None, 0], [5, 3, 0, None, 1]], buf=None, mode=9, extra=5)}


def region_base(fmt, px=4):
    """two 8 x 8 regions, blocks 0 .. 3 and 4 .. 7 of 100"""
    pitch = bpp_of(fmt, px)[0] * 8
    return dict(fmt=fmt, buf=SRC, total=100, regs=[[0, 8, 8, DST, pitch], [4, 8, 8, DST + 0x100000, pitch]], count=None, mode=1, extra=0)


def region_array(s, keep):
    if s["regs"] is None:
        return None, (2 if s["count"] is None else s["count"])
    arr = (Region * max(1, len(s["regs"])))(*[Region(*r) for r in s["regs"]])
    keep.append(arr)
    return arr, (len(s["regs"]) if s["count"] is None else s["count"])


def region_args(kind, has_mode, s, keep):
    arr, count = region_array(s, keep)
    head = [] if s["fmt"] is None else [s["fmt"]]
    settings = [s["mode"], True, False] if has_mode else []
    if kind == "plan":
        return [s["total"], arr, count, None, 0]
    if kind == "host":
        bs = 8 if s["fmt"] in (1, 4) else 16
        return head + [s["buf"], s["total"] * bs + s["extra"], arr, count] + settings
    return head + [s["buf"], s["total"], arr, count] + settings + [None]


def region_scenarios(fmt, kind, has_mode, px=4):
    """(case name, scenario, has nothing to do)"""
    for name, change in region_nothing().items():
        s = region_base(fmt, px)
        change(s)
        yield name, s, True
    defects = region_defects(fmt, kind, has_mode, px)
    for names in [(n,) for n in defects] + list(itertools.combinations(defects, 2)) + [tuple(defects)]:
        s = region_base(fmt, px)
        # (a list that is NULL has no regions to spoil)
        for n in sorted(names, key=lambda n: n == "regions"):
            defects[n](s)
        yield " + ".join(names), s, False
    for name, change in region_variants(fmt, kind, has_mode, px).items():
        s = region_base(fmt, px)
        change(s)
        yield name, s, False


def region_cases(keep):
    for call, kind, fmts, has_mode, px in REGION_CALLS:
        for fmt in fmts:
            tag = "" if fmt is None else f"format {fmt}: "
            for name, s, nothing in region_scenarios(fmt, kind, has_mode, px):
                yield call, tag + name, region_args(kind, has_mode, s, keep), nothing


def batch_cases(keep):
    def item(bc7, s):
        arr, count = region_array(s, keep)
        if bc7:
            return Bc7BatchItem(s["buf"], s["total"], arr, count, 0)
        return BatchItem(s["buf"], s["total"], arr, count, s["fmt"] & 0xFF, s["mode"], 1, 0)

    for bc7, call, hook in ((False, "dxtlt_untransform_decode_images_batch_device", "dxtlt_debug_plan_image_batch"),
                            (True, "dxtlt_untransform_decode_bc7_images_batch_device", "dxtlt_debug_plan_bc7_image_batch")):
        kind_of_item = Bc7BatchItem if bc7 else BatchItem

        def both(name, items, count, nothing):
            arr = None if items is None else (kind_of_item * max(1, len(items)))(*items)
            keep.append(arr)
            yield call, name, [arr, count, None], nothing
            yield hook, name, [arr, count, None, 0], nothing

        yield from both("nothing to do, no items", None, 0, True)
        yield from both("NULL item array", None, 3, False)
        for fmt in ((None,) if bc7 else (1, 3, 4, 5)):
            tag = "" if fmt is None else f"format {fmt}: "
            good = region_base(fmt)
            for name, s, nothing in region_scenarios(fmt, "fused", not bc7):
                if nothing:
                    yield from both(tag + name, [item(bc7, s), item(bc7, s)], 2, True)
                    continue
                # the defective item in the middle of three and in front
                yield from both(tag + "item 1: " + name, [item(bc7, good), item(bc7, s), item(bc7, good)], 3, False)
                yield from both(tag + "item 0: " + name, [item(bc7, s), item(bc7, good)], 2, False)
            # the first defective item is the answer, whatever the kinds of defect
            late, early = region_base(fmt), region_base(fmt)
            late["regs"][1][0] = 2
            early["regs"] = None
            yield from both(tag + "order in item 1, regions in item 2", [item(bc7, good), item(bc7, late), item(bc7, early)], 3, False)


def other_cases():
    for name in ("dxtlt_decode_bc7_blocks", "dxtlt_decode_bc6h_blocks"):
        out = 64 if "bc7" in name else 128
        for call, tail in ((name, []), (name + "_device", [None])):
            yield call, "nothing to do, no blocks", [None, 0, None, 0] + tail, True
            yield call, "len", [SRC, 16 * 3 + 5, DST, out * 4] + tail, False
            yield call, "len + null", [None, 16 * 3 + 5, DST, out * 4] + tail, False
            yield call, "len + pixels_len", [SRC, 16 * 3 + 5, DST, 0] + tail, False
            yield call, "null", [None, 16 * 3, DST, out * 3] + tail, False
            yield call, "null pixels", [SRC, 16 * 3, None, out * 3] + tail, False
            yield call, "null + pixels_len", [None, 16 * 3, DST, out * 3 - 1] + tail, False
            yield call, "pixels_len", [SRC, 16 * 3, DST, out * 3 - 1] + tail, False
            yield call, "pixels_len zero", [SRC, 16, DST, 0] + tail, False
    for call, tail in (("dxtlt_image_mip_level", [None] * 5), ("dxtlt_image_mip_chain", [None])):
        for name, (w, h, mips, x) in {"zero width": (0, 8, 1, 0), "zero height": (8, 0, 1, 0), "zero mip_count": (8, 8, 0, 0)}.items():
            yield call, name, [w, h, mips, x] + ([None] if "chain" in call else []) + tail, False
    yield "dxtlt_image_mip_level", "level past the chain", [8, 8, 3, 3] + [None] * 5, False
    yield "dxtlt_image_mip_level", "nothing to write", [8, 8, 3, 2] + [None] * 5, True
    yield "dxtlt_image_mip_chain", "null regions", [8, 8, 3, 0, None, None], False


def cases(keep):
    """(call, case, arguments, whether the call has nothing to do) of every case; `keep` holds what the arguments point to"""
    yield from image_cases()
    yield from region_cases(keep)
    yield from batch_cases(keep)
    yield from other_cases()


def run(lib):
    """[call, case, return code, error text] of every case, in order; the text of a call that succeeds is ''"""
    rows, seen, keep = [], set(), []
    for call, case, args, nothing in cases(keep):
        assert (call, case) not in seen, (call, case)
        seen.add((call, case))
        rc = getattr(lib, call)(*args)
        text = lib.dxtlt_last_error().decode() if rc != 0 else ""
        # a case with a defect never gets as far as a device: invalid length, invalid argument or a hook's -1, nothing else
        assert rc in (1, 2, -1) or nothing, (call, case, rc, text)
        assert rc == 0 or not nothing, (call, case, rc, text)
        rows.append([call, case, rc, text])
    return rows


GROUP = re.compile(r"^((?:format -?\d+: )?(?:item \d+: )?)(.*)$")   # what a case's name starts with: its format and batch item


def answer(rc, text):
    return f"{rc}: {text}" if text else str(rc)


def table_of(rows):
    """{call: {group: {"return code: error text": [cases]}}}, everything in the order of its first appearance; a case's name is
    its group, ": " and the name listed here"""
    table = {}
    for call, case, rc, text in rows:
        group, name = GROUP.match(case).groups()
        table.setdefault(call, {}).setdefault(group[:-2], {}).setdefault(answer(rc, text), []).append(name)
    return table


def answers_of(table):
    """{(call, case): answer} of a table"""
    return {(call, (group + ": " if group else "") + name): a
            for call, groups in table.items() for group, answers in groups.items() for a, names in answers.items() for name in names}


def dump(table):
    """the table as JSON, one line per answer"""
    calls = []
    for call, groups in table.items():
        parts = []
        for group, answers in groups.items():
            lines = ",\n".join(f"   {json.dumps(a)}: {json.dumps(names)}" for a, names in answers.items())
            parts.append(f"  {json.dumps(group)}: {{\n{lines}\n  }}")
        calls.append(f" {json.dumps(call)}: {{\n" + ",\n".join(parts) + "\n }")
    return "{\n" + ",\n".join(calls) + "\n}\n"


def main():
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import dxt_lossless_transform_amd as pkg

    rows = run(load(pkg._lib.lib_path()))
    with open(TABLE, "w") as f:
        f.write(dump(table_of(rows)))
    print(f"{len(rows)} cases of {len({r[0] for r in rows})} calls -> {TABLE}")


if __name__ == "__main__":
    main()
