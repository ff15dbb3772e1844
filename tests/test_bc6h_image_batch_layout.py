"""The host side of dxtlt_untransform_decode_bc6h_images_batch_device (include/dxtlt_bc6h_image.h, "many buffers in one call"), on
a machine without a GPU: every check in its documented order with the defective item first, in the middle and last; the planning
hook dxtlt_debug_plan_bc6h_image_batch against a plain Python statement of the plan, against the single call's plan of every item
and -- the host side is written once for both formats -- record for record against the BC7 hook's plan of the same lists; the
limit of a launch; the generic batch call still refusing BC6H and BC7; the Python and C++ wrappers.  Addresses are numbers: nothing
is dereferenced."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bc7_image_batch_common as bc7
from bc6h_image_batch_common import MAX_WGS, BatchItem, Item, PlannedEntry, batch_items, load, made_up, plan, plan_of
from bc6h_image_regions_common import BPP, GRANULE, THREE_FACES, TOTAL_THREE, Launch, groups_of
from image_regions_common import CHAIN_256, E_ARGUMENT, OK, PER_LAUNCH, Region, TOTAL_256, blocks_of, mip_chain, region_array, region_end

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_64, TOTAL_64 = mip_chain(64, 64, 7)
assert TOTAL_64 == 343


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


def last_error(lib):
    return lib.dxtlt_last_error().decode()


# ---- the checks -----------------------------------------------------------------------------------------------------------
# the single call's checks in the single call's documented order: (name, text the error carries)
DEFECTS = [("regions", "NULL regions"), ("buffer", "NULL buffer"), ("pixels", "NULL pixels"), ("small pitch", "pitch is smaller"),
           ("multiple", "multiples of"), ("range", "exceeds total_blocks"), ("order", "ascending")]


def defective_item(defects, keep):
    """an item of two 8 x 8 regions in 100 blocks with the named defects"""
    buffer = 0x10000
    regs = (Region * 2)(Region(0, 8, 8, 0x20000, 64), Region(4, 8, 8, 0x30000, 64))
    if "buffer" in defects:
        buffer = None
    if "pixels" in defects:
        regs[0].pixels = None
    if "small pitch" in defects:
        regs[0].pitch = 56
    if "multiple" in defects:
        regs[0].pixels = None if "pixels" in defects else 0x20004   # a multiple of 4, which RGBA8888 takes and RGBA16F does not
    if "range" in defects:
        regs[0].first_block = 98
    if "order" in defects:
        regs[1].first_block = 2
    keep.append(regs)
    return BatchItem(buffer, 100, None if "regions" in defects else regs, 2, 0)


def good_items(keep):
    """five ordinary items of different sizes"""
    items = [Item(TOTAL_256, list(CHAIN_256)), Item(TOTAL_64, list(CHAIN_64)), Item(2391, [(1000, 64, 64)]), Item(1024, [(0, 128, 128)]),
             Item(TOTAL_THREE, list(THREE_FACES))]
    return batch_items(items, *made_up(items), keep)


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
        assert lib.dxtlt_untransform_decode_bc6h_images_batch_device(arr, 5, None) == E_ARGUMENT, (name, extra)
        err = last_error(lib)
        assert text in err and f"bc6h image batch item {where}:" in err, (name, extra, err)
        # nothing was enqueued (there is no device here to enqueue on), and the hook refuses the batch too
        assert lib.dxtlt_debug_plan_bc6h_image_batch(arr, 5, None, 0) == -1


def test_a_pitch_of_four_bytes_a_pixel_is_too_small(lib):
    keep = []
    arr = good_items(keep)
    regs = (Region * 1)(Region(0, 8, 8, 0x20000, 32))
    keep.append(regs)
    arr[1] = BatchItem(0x10000, 100, regs, 1, 0)
    assert lib.dxtlt_untransform_decode_bc6h_images_batch_device(arr, 5, None) == E_ARGUMENT
    assert "pitch is smaller" in last_error(lib) and "bc6h image batch item 1:" in last_error(lib)


def test_the_first_defective_item_is_the_answer(lib):
    keep = []
    arr = good_items(keep)
    arr[3] = defective_item(["pixels"], keep)       # an early kind of defect in a later item
    arr[1] = defective_item(["order"], keep)        # the last kind in an earlier one
    assert lib.dxtlt_untransform_decode_bc6h_images_batch_device(arr, 5, None) == E_ARGUMENT
    assert "item 1:" in last_error(lib) and "ascending" in last_error(lib)


def test_empty_batches_and_items_without_regions(lib):
    assert lib.dxtlt_untransform_decode_bc6h_images_batch_device(None, 0, None) == OK
    assert lib.dxtlt_untransform_decode_bc6h_images_batch_device(None, 3, None) == E_ARGUMENT
    assert "NULL item array" in last_error(lib)
    assert lib.dxtlt_debug_plan_bc6h_image_batch(None, 3, None, 0) == -1 and lib.dxtlt_debug_plan_bc6h_image_batch(None, 0, None, 0) == 0
    # an item without a non-empty region is skipped: its buffer pointer and the place of its regions are not looked at
    regs = (Region * 2)(Region(2**63, 0, 7, None, 0), Region(5, 3, 0, None, 1))
    arr = (BatchItem * 2)(BatchItem(None, 0, regs, 2, 0), BatchItem(None, 0, None, 0, 0))
    assert lib.dxtlt_debug_plan_bc6h_image_batch(arr, 2, None, 0) == 0
    assert lib.dxtlt_untransform_decode_bc6h_images_batch_device(arr, 2, None) == OK
    # ... also between two ordinary items, where it owns no entry
    items = [Item(TOTAL_64, list(CHAIN_64)), Item(0, [(2**63, 0, 7), (5, 3, 0)]), Item(TOTAL_64, list(CHAIN_64))]
    addresses, pointers = made_up(items)
    addresses[1] = None
    assert [e[0] for e in plan(lib, items, addresses, pointers)] == [0, 2]


def test_the_generic_batch_call_still_refuses_formats_6_and_7(pkg):
    import image_batch_common as generic

    g = generic.load(pkg)
    for fmt in (6, 7):
        regs = (Region * 1)(Region(0, 8, 8, 0x20000, 64))
        arr = (generic.BatchItem * 1)(generic.BatchItem(0x10000, 100, regs, 1, fmt, 0, 0, 0))
        assert g.dxtlt_untransform_decode_images_batch_device(arr, 1, None) == E_ARGUMENT
        assert "format must be" in g.dxtlt_last_error().decode()


# ---- the plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1, 37, 1023, 1024, 1025, 2391, 5463])
def test_plan_of_every_total(lib, total):
    main = total - total % GRANULE
    for regions in ([(0, 4, 4 * total)], [(total - 1, 1, 1)], [(0, 2, 3), (total - 1, 4, 4)] if total > 1 else [(0, 2, 3)]):
        items = [Item(total, regions)]
        got = plan(lib, items)
        assert got == plan_of(items), (total, regions)
        (e,) = got
        first, end = regions[0][0], region_end(regions[-1])
        assert e[4] == (0 if first >= main else (min(end, main) - 1) // GRANULE - first // GRANULE + 1)
        assert (e[6] >= 0) == (end > main)


def test_plan_of_the_chains(lib):
    # the 256 x 256 nine-level chain: 5 granules and the tail part
    assert plan(lib, [Item(TOTAL_256, list(CHAIN_256))]) == [(0, 0, 9, 0, 5, 0, 0, 5, 1)]
    # a 64 x 64 chain is the tail part alone: the granule launch is empty
    assert plan(lib, [Item(TOTAL_64, list(CHAIN_64))]) == [(0, 0, 7, 0, 0, 0, 0, 0, 1)]
    # a range wholly inside the main part: no tail entry
    assert plan(lib, [Item(TOTAL_256, CHAIN_256[:2])]) == [(0, 0, 2, 0, 5, 0, -1, 5, 0)]
    assert plan(lib, [Item(2391, [(1500, 16, 4)])]) == [(0, 0, 1, 1, 1, 0, -1, 1, 0)]
    assert plan(lib, [Item(2391, [(2044, 16, 4)])]) == [(0, 0, 1, 1, 1, 0, -1, 1, 0)]
    assert plan(lib, [Item(2391, [(2044, 20, 4)])]) == [(0, 0, 1, 1, 1, 0, 0, 1, 1)]
    # the three together: first_wg and the tail index count up in list order
    items = [Item(TOTAL_256, list(CHAIN_256)), Item(TOTAL_64, list(CHAIN_64)), Item(TOTAL_256, CHAIN_256[:2]), Item(TOTAL_256, list(CHAIN_256))]
    assert plan(lib, items) == [(0, 0, 9, 0, 5, 0, 0, 15, 3), (1, 0, 7, 0, 0, 5, 1, 15, 3), (2, 0, 2, 0, 5, 5, -1, 15, 3),
                                (3, 0, 9, 0, 5, 10, 2, 15, 3)] == plan_of(items)


def test_plan_of_an_item_of_two_entries_that_share_a_granule(lib):
    # 20 regions of 205 blocks: the groups are regions 0 .. 15 (blocks 0 .. 3279) and 16 .. 19 (3280 .. 4099); granule 3 is in both
    regions = [(205 * k, 164, 20) for k in range(20)]
    assert blocks_of(164, 20) == 205 and [len(g) for _, g in groups_of(regions)] == [PER_LAUNCH, 4]
    items = [Item(4101, regions)]
    got = plan(lib, items)
    assert got == [(0, 0, 16, 0, 4, 0, -1, 5, 1), (0, 16, 4, 3, 1, 4, 0, 5, 1)] == plan_of(items)
    # three faces of a 128 chain: two groups that share granule 2, the second reaches the tail part
    items = [Item(TOTAL_THREE, list(THREE_FACES))]
    assert plan(lib, items) == [(0, 0, 16, 0, 3, 0, -1, 5, 1), (0, 16, 8, 2, 2, 3, 0, 5, 1)] == plan_of(items)


def test_plan_with_gaps_and_empty_regions(lib):
    # a group is not split at a gap: blocks 0 and 4000 of the chain's buffer are granules 0 .. 3
    assert plan(lib, [Item(TOTAL_256, [(0, 4, 4), (4000, 4, 4)])]) == [(0, 0, 2, 0, 4, 0, -1, 4, 0)]
    # empty regions are no part of a group, wherever their first_block points; the group's index is that of its first real region
    regions = [(2**63, 0, 7), CHAIN_256[0], (2**63, 5, 0), CHAIN_256[2], (5400, 0, 0), CHAIN_256[5]]
    items = [Item(TOTAL_256, regions), Item(TOTAL_256, [(2**63, 0, 7)]), Item(TOTAL_256, [])]
    assert plan(lib, items) == [(0, 1, 3, 0, 5, 0, 0, 5, 1)] == plan_of(items)
    # seventeen real regions between empty ones: the second group starts at the seventeenth real region
    regions = []
    for k in range(17):
        regions += [(7, 0, 0), (3 * k, 4, 4)]
    items = [Item(100, regions)]
    assert [e[:3] for e in plan(lib, items)] == [(0, 1, 16), (0, 33, 1)] and plan(lib, items) == plan_of(items)


def mixed_items(count, seed):
    """`count` items of mixed sizes and region layouts: whole chains, tail-only chains, single regions anywhere, lists of many
    small regions with gaps, items without regions"""
    rng = np.random.default_rng(seed)
    items = []
    for i in range(count):
        kind = i % 6
        if kind == 0:
            items.append(Item(TOTAL_256, list(CHAIN_256)))
        elif kind == 1:
            items.append(Item(TOTAL_64, list(CHAIN_64)))
        elif kind == 2:
            total = int(rng.integers(1, 9000))
            n = int(rng.integers(1, total + 1))
            first = int(rng.integers(0, total - n + 1))
            items.append(Item(total, [(first, 4, 4 * n)]))
        elif kind == 3:
            n = int(rng.integers(1, 40))
            regions, at = [], int(rng.integers(0, 3000))
            for _ in range(n):
                w, h = int(rng.integers(1, 200)), int(rng.integers(1, 60))
                regions.append((at, w, h))
                at += blocks_of(w, h) + int(rng.integers(0, 3)) * int(rng.integers(0, 700))
            items.append(Item(at + int(rng.integers(0, 1500)), regions))
        elif kind == 4:
            items.append(Item(int(rng.integers(0, 5000)), [(2**63, 0, 3)] if i % 12 == 4 else []))
        else:
            total = 1024 * int(rng.integers(1, 6))
            items.append(Item(total, [(0, 128, 32 * (total // 1024))]))
    return items


def test_plan_of_200_mixed_items(lib):
    items = mixed_items(200, 7)
    got = plan(lib, items)
    assert got is not None and got == plan_of(items)
    # first_wg ascending and contiguous, the launch totals, and at most two launches: every entry reports the same two totals
    at, tails = 0, 0
    for e in got:
        assert e[5] == at
        at += e[4]
        if e[6] >= 0:
            assert e[6] == tails
            tails += 1
    assert {e[7:] for e in got} == {(at, tails)} and at > 0 and tails > 0
    assert any(e[4] == 0 for e in got) and any(e[6] < 0 for e in got) and len({e[0] for e in got}) < len(got)


def test_every_item_is_planned_as_the_single_call_plans_it(lib):
    items = mixed_items(200, 11) + [Item(4101, [(205 * k, 164, 20) for k in range(20)])]
    got = plan(lib, items)
    for i, it in enumerate(items):
        mine = [e for e in got if e[0] == i]
        arr = region_array(it.regions, [0x7000000000 + 0x100000 * k for k in range(len(it.regions))], [BPP * r[1] for r in it.regions])
        out = (Launch * 64)()
        n = lib.dxtlt_debug_plan_bc6h_images(it.total, arr, len(it.regions), out, 64)
        assert 0 <= n <= 64
        alone = [(o.first_region, o.region_count, o.first_granule, o.granule_count, o.tail) for o in out[:n]]
        want = []
        for e in mine:
            if e[4]:
                want.append((e[1], e[2], e[3], e[4], 0))
            if e[6] >= 0:
                want.append((e[1], e[2], (it.total - it.total % GRANULE) // GRANULE, 1, 1))
        assert alone == want, (i, it.total, it.regions)


def test_the_plan_is_the_bc7_calls_plan_record_for_record(pkg, lib):
    """the same item lists, each in its format's layout (pitch 8 w here, 4 w there): what "written once" promises"""
    bc7_lib = bc7.load(pkg)
    lists = [mixed_items(200, 7), mixed_items(200, 11), [Item(4101, [(205 * k, 164, 20) for k in range(20)])],
             [Item(TOTAL_THREE, list(THREE_FACES)), Item(TOTAL_64, list(CHAIN_64))],
             [Item(TOTAL_256, [(2**63, 0, 7), CHAIN_256[0], (2**63, 5, 0), CHAIN_256[2], (5400, 0, 0), CHAIN_256[5]]), Item(0, [])],
             [Item(1 << 34, [(0, 1 << 19, 1 << 19)])]]
    lists += [[Item(total, [(0, 4, 4 * total)]), Item(total, [(total - 1, 1, 1)])] for total in (1, 37, 1023, 1024, 1025, 2391, 5463)]
    for items in lists:
        theirs = bc7.plan(bc7_lib, [bc7.Item(*it) for it in items])
        assert plan(lib, items) == theirs, items[:2]
    assert bc7.plan(bc7_lib, [bc7.Item(*it) for it in lists[5]]) is None and len(bc7.plan(bc7_lib, [bc7.Item(*it) for it in lists[0]])) > 100
    assert ctypes.sizeof(PlannedEntry) == ctypes.sizeof(bc7.PlannedEntry) and PlannedEntry._fields_ == bc7.PlannedEntry._fields_


def test_plan_counts_beyond_the_capacity(lib):
    items = [Item(TOTAL_THREE, list(THREE_FACES)), Item(TOTAL_64, list(CHAIN_64))]
    keep = []
    arr = batch_items(items, *made_up(items), keep)
    assert lib.dxtlt_debug_plan_bc6h_image_batch(arr, 2, None, 0) == 3
    out = (PlannedEntry * 2)()
    assert lib.dxtlt_debug_plan_bc6h_image_batch(arr, 2, out, 2) == 3 and (out[1].first_region, out[1].first_granule) == (16, 2)


# ---- the limit ------------------------------------------------------------------------------------------------------------
def test_a_launch_of_2_to_the_24_workgroups_is_refused(lib):
    # one region of 2^19 x 2^19 pixels: 2^34 blocks, 2^24 granules
    big = Item(1 << 34, [(0, 1 << 19, 1 << 19)])
    keep = []
    arr = batch_items([big], *made_up([big]), keep)
    assert lib.dxtlt_debug_plan_bc6h_image_batch(arr, 1, None, 0) == -1 and plan_of([big]) is None
    assert lib.dxtlt_untransform_decode_bc6h_images_batch_device(arr, 1, None) == E_ARGUMENT
    assert "16777215 granules" in last_error(lib) and "tail parts" in last_error(lib) and "bc6h image batch item 0:" in last_error(lib)
    # one granule fewer, as two items: 2^24 - 2 granules and one
    most = Item(2048 * ((1 << 23) - 1), [(0, 4 * 2048, 4 * ((1 << 23) - 1))])
    one = Item(1024, [(0, 128, 128)])
    got = plan(lib, [most, one])
    assert got == plan_of([most, one]) and [e[4] for e in got] == [MAX_WGS - 1, 1] and got[1][5] == MAX_WGS - 1
    # ... and one more granule is one too many, wherever the item stands: the item that crosses the limit is named
    items = [one, most, one]
    arr = batch_items(items, *made_up(items), keep)
    assert lib.dxtlt_untransform_decode_bc6h_images_batch_device(arr, 3, None) == E_ARGUMENT and "item 2:" in last_error(lib)
    # tail parts do not count against the granules
    tails = [Item(TOTAL_64, list(CHAIN_64))] * 3
    assert [e[6] for e in plan(lib, [most, one] + tails)] == [-1, -1, 0, 1, 2]


# ---- Python and C++ ---------------------------------------------------------------------------------------------------------
def test_python_module_exposes_the_bc6h_batch_call(pkg):
    from dxt_lossless_transform_amd import image

    assert image.untransform_decode_bc6h_images_batch([]) == []
    with pytest.raises(TypeError):
        image.untransform_decode_bc6h_images_batch([(np.zeros(16, np.uint8), [(0, 4, 4)])])   # device tensors only
    with pytest.raises(pkg.InvalidLength):
        image.untransform_decode_bc6h_images_batch([(np.zeros(17, np.uint8), [(0, 4, 4)])])
    assert ctypes.sizeof(image.Bc6hImageBatchItem) == ctypes.sizeof(BatchItem) == 32
    # the BC7 wrapper, which shares its body, is what it was
    assert image.untransform_decode_bc7_images_batch([]) == []
    with pytest.raises(TypeError, match="untransform_decode_bc7_images_batch takes device tensors"):
        image.untransform_decode_bc7_images_batch([(np.zeros(16, np.uint8), [(0, 4, 4)])])


def test_cpp_wrapper_compiles_links_and_checks_its_arguments(pkg, tmp_path):
    libdir = os.path.dirname(pkg._lib.lib_path())
    exe = str(tmp_path / "test_cpp_bc6h_image_batch")
    src = os.path.join(ROOT, "tests", "cpp", "test_cpp_bc6h_image_batch.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, src, f"-L{libdir}", "-ldxtlt_gfx950",
                           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
