"""The return code and dxtlt_last_error() text of every single defect of dxtlt_untransform_decode_bc6h_images_batch_device and of
its planning hook (include/dxtlt_bc6h_image.h, "many buffers in one call"), on a machine without a GPU.  The cases are the ones
tests/golden/make_image_call_defects.py lists for the BC7 batch call -- each defect alone, every pair, all together, the variants,
the calls with nothing to do, in item 1 of three and in item 0 of two -- made with RGBA16F's numbers (an 8-byte pixel: pitch 64,
too small at 56, the pointer off by 4).  The answers are the BC7 batch call's RECORDED ones in tests/golden/image_call_defects.json
with two replacements: "bc7" becomes "bc6h", and the two texts of the 4-byte pixel's rule become the 8-byte pixel's.  The table and
its generator are not regenerated: both formats' calls are one body (csrc/granule_image_batch_api.h), and this is what holds the
second family to the first one's record."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from bc6h_image_batch_common import BatchItem, load
from image_regions_common import Region

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BC7_CALL, BC7_HOOK = "dxtlt_untransform_decode_bc7_images_batch_device", "dxtlt_debug_plan_bc7_image_batch"
CALL, HOOK = "dxtlt_untransform_decode_bc6h_images_batch_device", "dxtlt_debug_plan_bc6h_image_batch"
# csrc/image_host.h: kRgba8888's two texts -> kRgba16f's
RULE_TEXTS = {"pitch is smaller than 4 * width": "pitch is smaller than 8 * width",
              "pitch and the pixel pointer must be multiples of 4": "pitch and the pixel pointer must be multiples of 8"}


@pytest.fixture(scope="module")
def make():
    spec = importlib.util.spec_from_file_location("make_image_call_defects", os.path.join(GOLDEN, "make_image_call_defects.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


def bc6h_cases(make, keep):
    """(hook?, case name, items or None, count) -- make.batch_cases' BC7 branch with an 8-byte pixel"""
    def item(s):
        if s["regs"] is None:
            arr, count = None, (2 if s["count"] is None else s["count"])
        else:
            arr = (Region * max(1, len(s["regs"])))(*[Region(*r) for r in s["regs"]])
            keep.append(arr)
            count = len(s["regs"]) if s["count"] is None else s["count"]
        return BatchItem(s["buf"], s["total"], arr, count, 0)

    yield "nothing to do, no items", None, 0
    yield "NULL item array", None, 3
    good = make.region_base(None, 8)
    assert good["regs"][0][4] == 64
    for name, s, nothing in make.region_scenarios(None, "fused", False, 8):
        if nothing:
            yield name, [item(s), item(s)], 2
            continue
        yield "item 1: " + name, [item(good), item(s), item(good)], 3
        yield "item 0: " + name, [item(s), item(good)], 2
    late, early = make.region_base(None, 8), make.region_base(None, 8)
    late["regs"][1][0] = 2
    early["regs"] = None
    yield "order in item 1, regions in item 2", [item(good), item(late), item(early)], 3


def translated(answer):
    answer = answer.replace("bc7", "bc6h")
    for old, new in RULE_TEXTS.items():
        answer = answer.replace(old, new)
    return answer


def test_every_answer_is_the_bc7_batch_calls_recorded_one(make, lib):
    with open(make.TABLE) as f:
        recorded = make.answers_of(json.load(f))
    want = {(call, case): translated(a) for (call, case), a in recorded.items() if call in (BC7_CALL, BC7_HOOK)}
    assert any("bc6h image batch item 1:" in a for a in want.values()) and not any("bc7" in a for a in want.values())
    keep, got = [], {}
    for case, items, count in bc6h_cases(make, keep):
        arr = None if items is None else (BatchItem * max(1, len(items)))(*items)
        keep.append(arr)
        for mine, theirs, args in ((CALL, BC7_CALL, [arr, count, None]), (HOOK, BC7_HOOK, [arr, count, None, 0])):
            rc = getattr(lib, mine)(*args)
            text = lib.dxtlt_last_error().decode() if rc != 0 else ""
            # no case gets as far as a device
            assert rc in (0, 2, -1), (mine, case, rc, text)
            assert (theirs, case) not in got
            got[(theirs, case)] = make.answer(rc, text)
    different = [(k, got[k], want.get(k)) for k in got if got[k] != want.get(k)]
    assert not different, different[:10]
    assert set(got) == set(want), "the cases are not the ones recorded for the BC7 batch call"
    # every single defect of the documented order is among them, in item 0 and in item 1, with an answer of its own kind
    for n in ("regions", "buffer", "pixels", "small pitch", "multiple", "range", "order"):
        for where in (0, 1):
            a = got[(BC7_CALL, f"item {where}: {n}")]
            assert a.startswith("2: ") and f"bc6h image batch item {where}: " in a, (n, where, a)
            assert got[(BC7_HOOK, f"item {where}: {n}")] == "-1: " + a[3:]


def test_the_eight_byte_pixel_is_the_rule_applied(lib):
    """what the BC7 call takes and this one must refuse, and the other way round: a pitch of 4 * width, and a pointer and pitch
    that are multiples of 4 only"""
    def call(pixels, pitch, width=8):
        regs = (Region * 1)(Region(0, width, 8, pixels, pitch))
        arr = (BatchItem * 1)(BatchItem(0x10000, 100, regs, 1, 0))
        rc = lib.dxtlt_debug_plan_bc6h_image_batch(arr, 1, None, 0)
        return rc, lib.dxtlt_last_error().decode()

    assert call(0x20000, 64)[0] == 1
    rc, text = call(0x20000, 32)
    assert rc == -1 and "pitch is smaller" in text
    rc, text = call(0x20004, 64)
    assert rc == -1 and "multiples of" in text
    rc, text = call(0x20000, 68)
    assert rc == -1 and "multiples of" in text
    assert call(0x20008, 72)[0] == 1
    assert C.sizeof(BatchItem) == 32
