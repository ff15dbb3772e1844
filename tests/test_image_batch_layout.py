"""The host side of dxtlt_untransform_decode_images_batch_device (include/dxtlt_image.h, "many buffers in one call"), on a machine
without a GPU: every check in its documented order with the defective item first, in the middle and last; the planning hook
dxtlt_debug_plan_image_batch for the shapes the issue names; and the proof that the batches of tests/test_image_batch_gpu.py
reach every tile form and every path of the workgroup lookup.  Addresses are numbers: nothing is dereferenced."""
import ctypes as C

import pytest

from image_batch_common import (ALIGNED_REGIONS, ALIGNED_TOTAL, GPU_BATCHES, SMALL, TILE, BatchItem, Item, batch_items, load,
                                many_regions, plan, reached)
from image_regions_common import (CHAIN_256, CUBE, E_ARGUMENT, FMTS, OK, PlannedLaunch, FMT_ID, Region, TOTAL_256, default_settings,
                                  other_settings)


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


def last_error(lib):
    return lib.dxtlt_last_error().decode()


# ---- the checks -----------------------------------------------------------------------------------------------------------
# the single call's checks in the single call's documented order: (name, text the error carries)
DEFECTS = [("format", "format must be"), ("regions", "NULL regions"), ("buffer", "NULL buffer"), ("pixels", "NULL pixels"),
           ("small pitch", "pitch is smaller"), ("multiple", "multiples of"), ("range", "exceeds total_blocks"),
           ("order", "ascending"), ("mode", "decorrelation_mode")]


def defective_item(defects, keep):
    """a BC1 item of two 8 x 8 regions with the named defects"""
    fmt, buffer, total, mode = 1, 0x10000, 100, 1
    regs = (Region * 2)(Region(0, 8, 8, 0x20000, 32), Region(4, 8, 8, 0x30000, 32))
    if "format" in defects:
        fmt = 9
    if "buffer" in defects:
        buffer = None
    if "pixels" in defects:
        regs[0].pixels = None
    if "small pitch" in defects:
        regs[0].pitch = 28
    if "multiple" in defects:
        regs[0].pixels = None if "pixels" in defects else 0x20002
    if "range" in defects:
        regs[0].first_block = 98
    if "order" in defects:
        regs[1].first_block = 2
    if "mode" in defects:
        mode = 4
    keep.append(regs)
    return BatchItem(buffer, total, None if "regions" in defects else regs, 2, fmt, mode, 0, 1)


def good_items(keep):
    """five ordinary items, one per format"""
    items = [Item(fmt, default_settings(fmt), TOTAL_256, list(CHAIN_256)) for fmt in FMTS]
    addresses = [0x1000000 * (i + 1) for i in range(5)]
    pointers = [[0x7000000000 + 0x10000000 * i + 0x100000 * k for k in range(len(CHAIN_256))] for i in range(5)]
    return batch_items(items, addresses, pointers, keep)


@pytest.mark.parametrize("where", [0, 2, 4])
@pytest.mark.parametrize("which", range(len(DEFECTS)))
def test_every_check_in_its_documented_order(lib, which, where):
    name, text = DEFECTS[which]
    later = [n for n, _ in DEFECTS[which + 1:]]
    # the defect alone, with the next one of the order, and with every later one: the earliest is the answer
    for extra in ([], later[:1], later):
        keep = []
        arr = good_items(keep)
        arr[where] = defective_item([name] + extra, keep)
        assert lib.dxtlt_untransform_decode_images_batch_device(arr, 5, None) == E_ARGUMENT, (name, extra)
        err = last_error(lib)
        assert text in err and f"item {where}:" in err, (name, extra, err)
        # nothing was enqueued (there is no device here to enqueue on), and the hook refuses the batch too
        assert lib.dxtlt_debug_plan_image_batch(arr, 5, None, 0) == -1


def test_empty_batches_and_items_without_regions(lib):
    assert lib.dxtlt_untransform_decode_images_batch_device(None, 0, None) == OK
    assert lib.dxtlt_untransform_decode_images_batch_device(None, 3, None) == E_ARGUMENT
    assert "NULL item array" in last_error(lib)
    assert lib.dxtlt_debug_plan_image_batch(None, 3, None, 0) == -1 and lib.dxtlt_debug_plan_image_batch(None, 0, None, 0) == 0
    # an item without a non-empty region is skipped: its buffer pointer, its mode and the place of its regions are not looked at
    regs = (Region * 2)(Region(2**63, 0, 7, None, 0), Region(5, 3, 0, None, 1))
    arr = (BatchItem * 2)(BatchItem(None, 0, regs, 2, 1, 9, 0, 0), BatchItem(None, 0, None, 0, 3, 9, 0, 0))
    assert lib.dxtlt_debug_plan_image_batch(arr, 2, None, 0) == 0
    assert lib.dxtlt_untransform_decode_images_batch_device(arr, 2, None) == OK


def test_a_launch_of_more_than_2_to_the_24_tiles_is_refused(lib):
    # 2^22 BC2 tiles per item: the fourth item would bring the launch to 2^24 workgroups
    total = 256 << 22
    keep = []
    items = [Item("bc2", default_settings("bc2"), total, [(0, 4 * 16384, 4 * 65536)]) for _ in range(4)]
    addresses = [0x100000000 * (i + 1) for i in range(4)]
    pointers = [[0x7000000000]] * 4
    assert len(plan(lib, items[:3], addresses[:3], pointers[:3])) == 3
    arr = batch_items(items, addresses, pointers, keep)
    assert lib.dxtlt_debug_plan_image_batch(arr, 4, None, 0) == -1
    assert lib.dxtlt_untransform_decode_images_batch_device(arr, 4, None) == E_ARGUMENT
    assert "16777215 tiles" in last_error(lib) and "item 3:" in last_error(lib)
    # ... of ONE format and settings: with other settings the fourth item has a launch of its own
    items[3] = items[3]._replace(settings=other_settings("bc2"))
    assert [e.launch for e in plan(lib, items, addresses, pointers)] == [0, 0, 0, 1]


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def shape(e):
    return (e.item, e.first_region, e.region_count, e.launch, e.first_wg, e.end_wg, e.full_tiles, e.form, e.first_block, e.range_blocks)


@pytest.mark.parametrize("fmt", FMTS)
def test_plan_of_a_256_chain(lib, fmt):
    (e,) = plan(lib, [Item(fmt, default_settings(fmt), TOTAL_256, list(CHAIN_256))])
    full = 5463 // TILE[fmt]
    # an odd block count: shifted tiles and an edge tile
    assert shape(e) == (0, 0, 9, 0, 0, full + 1, full, 0, 0, 5463)


@pytest.mark.parametrize("fmt", FMTS)
def test_plan_of_a_range_on_128_byte_lines_that_ends_on_a_tile(lib, fmt):
    regions = [(4096, 128, 128), (5120, 64, 64)] if TILE[fmt] == 256 else [(4096, 128, 128)]
    (e,) = plan(lib, [Item(fmt, default_settings(fmt), ALIGNED_TOTAL, regions)])
    blocks = 1280 if TILE[fmt] == 256 else 1024
    assert blocks % TILE[fmt] == 0
    assert shape(e) == (0, 0, len(regions), 0, 0, blocks // TILE[fmt], blocks // TILE[fmt], 1, 4096, blocks)


@pytest.mark.parametrize("fmt", FMTS)
def test_plan_of_a_range_on_128_byte_lines_that_does_not_end_on_a_tile(lib, fmt):
    (e,) = plan(lib, [Item(fmt, default_settings(fmt), ALIGNED_TOTAL, ALIGNED_REGIONS)])
    full = 1298 // TILE[fmt]
    assert 1298 % TILE[fmt] != 0
    assert shape(e) == (0, 0, 3, 0, 0, full + 1, full, 1, 4096, 1298)


@pytest.mark.parametrize("fmt", FMTS)
def test_plan_of_a_16_block_item(lib, fmt):
    (e,) = plan(lib, [Item(fmt, default_settings(fmt), 16, list(SMALL))])
    assert shape(e)[:7] == (0, 0, 1, 0, 0, 1, 0) and (e.first_block, e.range_blocks) == (0, 16)   # the edge tile alone


@pytest.mark.parametrize("count,entries", [(17, 2), (33, 3)])
def test_plan_of_more_regions_than_an_entry_holds(lib, count, entries):
    regions, total = many_regions(count)
    got = plan(lib, [Item("bc3", default_settings("bc3"), total, regions)])
    assert len(got) == entries
    assert [(e.first_region, e.region_count) for e in got] == [(16 * k, min(16, count - 16 * k)) for k in range(entries)]
    for k, e in enumerate(got):
        first, last = regions[16 * k], regions[min(count, 16 * k + 16) - 1]
        assert (e.first_block, e.range_blocks) == (first[0], last[0] + ((last[1] + 3) // 4) * ((last[2] + 3) // 4) - first[0])


def test_plan_of_a_cube_map(lib):
    got = plan(lib, [Item("bc1", default_settings("bc1"), 6 * 341, list(CUBE))])
    assert [(e.item, e.first_region, e.region_count, e.first_block) for e in got] == [(0, 0, 16, 0), (0, 16, 14, CUBE[16][0])]
    assert (got[0].range_blocks, got[1].range_blocks) == (CUBE[16][0], 6 * 341 - CUBE[16][0])   # the regions lie side by side


def test_plan_of_an_item_at_an_odd_address_goes_alone(lib):
    items = [Item("bc3", default_settings("bc3"), TOTAL_256, list(CHAIN_256)),
             Item("bc3", default_settings("bc3"), TOTAL_256, list(CHAIN_256), in_off=1),
             Item("bc3", default_settings("bc3"), TOTAL_256, list(CHAIN_256))]
    got = plan(lib, items)
    assert [e.launch for e in got] == [0, -1, 0]
    assert (got[1].first_wg, got[1].end_wg) == (0, 0) and got[2].first_wg == got[0].end_wg


def test_plan_empty_items_and_regions_own_nothing(lib):
    items = [Item("bc1", default_settings("bc1"), TOTAL_256, []),
             Item("bc1", default_settings("bc1"), TOTAL_256, [(0, 0, 8), (2**63, 5, 0)]),
             Item("bc1", default_settings("bc1"), TOTAL_256, [(0, 0, 8), CHAIN_256[1], (2**63, 0, 0), CHAIN_256[3]])]
    (e,) = plan(lib, items)
    assert (e.item, e.first_region, e.region_count) == (2, 1, 2)
    assert (e.first_block, e.range_blocks) == (4096, 5376 + 64 - 4096)


def test_plan_two_settings_of_one_format_are_two_launches(lib):
    items = [Item("bc3", s, TOTAL_256, list(CHAIN_256)) for s in (default_settings("bc3"), other_settings("bc3"), default_settings("bc3"))]
    got = plan(lib, items)
    assert [e.launch for e in got] == [0, 1, 0]
    assert [(e.first_wg, e.end_wg) for e in got] == [(0, 22), (0, 22), (22, 44)]


def test_plan_five_formats_are_five_launches_in_first_appearance_order(lib):
    order = ["bc4", "bc1", "bc5", "bc3", "bc2"]
    items = [Item(fmt, default_settings(fmt), TOTAL_256, list(CHAIN_256)) for fmt in order + order[::-1]]
    got = plan(lib, items)
    assert [e.launch for e in got] == [0, 1, 2, 3, 4, 4, 3, 2, 1, 0]
    # BC4 / BC5 ignore the decorrelation mode and the colour split: no launch of their own for them
    items = [Item("bc4", (0, True, False), 16, list(SMALL)), Item("bc4", (3, True, True), 16, list(SMALL))]
    assert [e.launch for e in plan(lib, items)] == [0, 0]


@pytest.mark.parametrize("name", sorted(GPU_BATCHES))
def test_workgroups_are_contiguous_and_forms_are_the_transform_plans(lib, name):
    items = GPU_BATCHES[name]()
    got = plan(lib, items)
    assert got is not None
    at = {}
    last_item = -1
    for e in got:
        assert e.item >= last_item   # list order
        last_item = e.item
        it = items[e.item]
        address = 0x10000000 + 0x100000 * e.item + it.in_off
        out = (PlannedLaunch * 8)()
        n = lib.dxtlt_debug_plan_transform(FMT_ID[it.fmt], 1, it.settings[0], int(it.settings[1]), int(it.settings[2]), address, 0,
                                           it.total, e.first_block, e.range_blocks, out, 8)
        assert 0 < n <= 8
        if e.launch < 0:
            # shifts that are no multiples of the element widths: the single call's shifted tiles, no workgroups of a batch launch
            assert out[0].kind == 2 and out[0].natural == 0 and (e.first_wg, e.end_wg, e.form) == (0, 0, 0)
            continue
        if e.full_tiles > 0:
            assert e.form == (1 if out[0].kind == 0 else 0), (name, e.item)
        else:
            # less than a tile: the transform's plan is its edge launch alone, whatever the form is called
            assert n == 1 and out[0].kind == 2 and out[0].workgroups == 1
        assert all(out[k].natural == 1 for k in range(n) if out[k].kind == 2)
        # workgroups: contiguous within a launch, in item order
        assert e.first_wg == at.get(e.launch, 0)
        tiles, rest = divmod(e.range_blocks, TILE[it.fmt])
        assert (e.full_tiles, e.end_wg) == (tiles, e.first_wg + tiles + (1 if rest else 0))
        at[e.launch] = e.end_wg
    for e in got:
        if e.launch >= 0:
            assert e.launch_wgs == at[e.launch]


def test_300_small_items_take_the_wide_index(lib):
    items = [Item("bc1", default_settings("bc1"), 16, list(SMALL)) for _ in range(300)]
    got = plan(lib, items)
    # more than 255 entries begin inside one 4096-workgroup span
    assert len(got) == 300 and all(e.wide_index == 1 and e.launch == 0 and e.end_wg == e.first_wg + 1 for e in got)
    assert all(e.wide_index == 0 for e in plan(lib, items[:255]))


# ---- what the GPU tests' batches reach ------------------------------------------------------------------------------------
def test_the_gpu_batches_reach_every_tile_form_and_lookup_path(lib):
    got = {name: reached(plan(lib, make())) for name, make in GPU_BATCHES.items()}
    everything = set().union(*got.values())
    assert everything == {"aligned tiles", "shifted tiles", "edge tiles", "bisection", "wide index", "multi-entry item", "alone",
                          "rotation"}
    assert {"wide index", "bisection", "rotation", "shifted tiles", "edge tiles"} <= got["many small"]
    assert {"aligned tiles", "shifted tiles", "edge tiles"} <= got["aligned"]
    assert "multi-entry item" in got["multi entry"] and "alone" in got["fallback"]
    # one launch of the aligned batch holds both forms
    entries = plan(lib, GPU_BATCHES["aligned"]())
    for launch in range(5):
        assert {e.form for e in entries if e.launch == launch and e.full_tiles > 0} == {0, 1}
    # the mixed batch: ten launches whose items are scattered over the list, the two empty items own nothing
    mixed = plan(lib, GPU_BATCHES["mixed"]())
    assert len({e.launch for e in mixed}) == 10 and len(mixed) == 40
    assert len({e.launch for e in plan(lib, GPU_BATCHES["every setting"]())}) == 36
    small = plan(lib, GPU_BATCHES["many small"]())
    assert len(small) == 606 and len({e.launch for e in small}) == 2
