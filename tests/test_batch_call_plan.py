"""What dxtlt_transform_batch_device enqueues for a whole batch, checked without a GPU through dxtlt_debug_plan_batch_call and
dxtlt_debug_plan_batch_granules (include/dxtlt_gfx950.h): the hooks run the call's own planner (plan_batch, csrc/batch_api.cpp) and
table writer on addresses that are only numbers.  Grouping, launch order, the uniform / strided decisions, the granule plans with
their coarse index, the layout of the one staged buffer, and that a defective batch is refused whole -- with the status codes the
two calls have always answered.  tests/test_batch_plan.py checks one launch's entries and workgroup index."""
import ctypes as C

import pytest

from bc7_image_batch_common import Item as Bc7ImageItem, load as load_bc7_image_batch, plan as bc7_image_plan, plan_of as bc7_image_plan_of

OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
GRANULES, TILES, SINGLE, PIXELS = 0, 1, 2, 3
BLOCK = {1: 8, 2: 16, 3: 16, 4: 8, 5: 16, 6: 16, 7: 16, 8: 4, 9: 3}
MAX_WGS = 0xFFFFFF
SRC, DST = 0x7F00_0000_0000, 0x7E00_0000_0000   # made-up device addresses on 4 KiB pages


class Planned(C.Structure):   # DxtltDebugPlannedEntry
    _fields_ = [("first_wg", C.c_uint32), ("end_wg", C.c_uint32), ("full_tiles", C.c_uint32), ("form", C.c_uint8),
                ("halo_vecs", C.c_uint8), ("shift", C.c_uint8 * 6), ("gbase", C.c_uint64 * 6)]


class Launch(C.Structure):   # DxtltDebugBatchLaunch
    _fields_ = [("kind", C.c_int32), ("format", C.c_int32), ("inverse", C.c_int32), ("settings_code", C.c_int32),
                ("items", C.c_uint32), ("entries", C.c_uint32), ("tails", C.c_uint32), ("workgroups", C.c_uint32),
                ("uniform_wgs", C.c_uint32), ("strided", C.c_uint32), ("wide", C.c_uint32), ("src_stride", C.c_int64),
                ("dst_stride", C.c_int64), ("table_offset", C.c_uint64), ("table_bytes", C.c_uint64), ("first_item", C.c_uint64)]


@pytest.fixture(scope="module")
def lib(pkg):
    from dxt_lossless_transform_amd.batch import DxtltBatchItem

    l = C.CDLL(pkg._lib.lib_path())
    items, sz, i32 = C.POINTER(DxtltBatchItem), C.c_size_t, C.c_int32
    l.dxtlt_debug_plan_batch_call.argtypes = [items, sz, i32, C.POINTER(Launch), sz, C.POINTER(C.c_uint64)]
    l.dxtlt_debug_plan_batch_granules.argtypes = [items, sz, i32, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), sz,
                                                  C.POINTER(C.c_uint32), sz]
    l.dxtlt_debug_plan_batch.argtypes = [i32] * 5 + [C.c_void_p] * 3 + [sz, C.c_void_p, C.c_void_p, sz, C.c_void_p]
    l.dxtlt_debug_plan_batch.restype = C.c_uint32
    l.dxtlt_transform_batch_device.argtypes = [items, sz, C.c_void_p]
    l.dxtlt_transform_batch_host.argtypes = [items, sz]
    l.dxtlt_last_error.restype = C.c_char_p
    l.Item = DxtltBatchItem
    return l


def item(lib, fmt, inverse, src, dst, blocks, mode=1, sa=1, sc=1):
    return lib.Item(src, dst, blocks * BLOCK[fmt], fmt, int(inverse), mode, sa, sc)


def array(lib, items):
    return (lib.Item * max(1, len(items)))(*items)


def call_plan(lib, items, pixels_allowed=0):
    """(the launches, the staged buffer's bytes); (None, 0) for a batch the call refuses"""
    arr, nbytes = array(lib, items), C.c_uint64(99)
    n = lib.dxtlt_debug_plan_batch_call(arr, len(items), pixels_allowed, None, 0, C.byref(nbytes))
    if n < 0:
        assert nbytes.value == 0
        return None, 0
    out = (Launch * max(1, n))()
    assert lib.dxtlt_debug_plan_batch_call(arr, len(items), pixels_allowed, out, n, C.byref(nbytes)) == n
    return list(out)[:n], nbytes.value


def group_alone(lib, fmt, inverse, mode, sa, sc, items):
    """dxtlt_debug_plan_batch for the buffers of `items` as one group: its workgroups, 0xFFFFFFFF when the kernel takes one not"""
    n = len(items)
    a = lambda v: (C.c_uint64 * n)(*v)
    out, index, wide = (Planned * n)(), (C.c_uint8 * (1 << 16))(), C.c_uint32(0)
    return lib.dxtlt_debug_plan_batch(fmt, int(inverse), mode, sa, sc, a([it.d_input for it in items]), a([it.d_output for it in items]),
                                      a([it.len // BLOCK[fmt] for it in items]), n, out, index, 1 << 16, C.byref(wide))


def effective_code(fmt, mode, sa, sc):
    """the settings code as the call has always grouped: what a format ignores does not tell two items apart (the arithmetic of
    format_has_colour / format_has_alpha_split, csrc/bcn_launch.h: colour endpoints in BC1..BC3, an alpha-endpoint split in BC3..BC5)"""
    colour, alpha = fmt in (1, 2, 3), fmt in (3, 4, 5)
    return ((mode if colour else 0) << 2) | ((1 if alpha and sa else 0) << 1) | (1 if colour and sc else 0)


def check_layout(launches, table_bytes):
    """offsets are multiples of 16, tables follow one another in launch order without overlap, the last one ends the buffer"""
    at = 0
    for l in launches:
        if l.kind in (GRANULES, TILES):
            assert l.table_offset % 16 == 0 and l.table_bytes % 16 == 0 and l.table_bytes > 0
            assert l.table_offset == at, (l.kind, l.format)
            at += l.table_bytes
        else:
            assert l.table_bytes == 0
    assert at == table_bytes


def mixed_batch(lib):
    """about twenty items: formats 1..7 in both directions, two settings combinations of BC1 and of BC3, an empty item, a BC1 item
    whose transformed side sits at 4 modulo 8 and one at 2 modulo 8.  Returns (items, (fmt, inverse, mode, sa, sc) per item)."""
    specs = []
    for fmt in (3, 7, 1, 5, 6, 2, 4):
        for inverse in (True, False):
            specs.append((fmt, inverse, 1, 1, 1))
    specs += [(1, False, 0, 0, 0), (3, True, 2, 0, 1), (3, False, 2, 0, 1), (1, False, 1, 1, 1), (3, True, 1, 1, 1)]
    items, at = [], 0
    for k, (fmt, inverse, mode, sa, sc) in enumerate(specs):
        blocks = [700, 2048 + 5, 1024, 7, 3 * 1024 + 1][k % 5] if fmt in (6, 7) else 100 + 613 * k
        items.append(item(lib, fmt, inverse, SRC + at, DST + at, blocks, mode, sa, sc))
        at += (blocks * 16 + 4095) // 4096 * 4096
    items.append(item(lib, 2, False, SRC + at, DST + at, 0))
    specs.append((2, False, 1, 1, 1))
    for off in (4, 2):   # the transformed side: the output of a forward item
        items.append(item(lib, 1, False, SRC + at, DST + at + off, 1000))
        specs.append((1, False, 1, 1, 1))
        at += 8192
    return items, specs


def test_launch_order_and_grouping(lib):
    items, specs = mixed_batch(lib)
    # which of the two odd BC1 items leave the batch kernel is the old hook's word: 4 modulo 8 keeps every stream of a BC1 buffer on
    # its element width (2, 2, 4 bytes), 2 modulo 8 takes the 4-byte index stream off it
    alone = [group_alone(lib, 1, False, 1, 1, 1, [it]) == 0xFFFFFFFF for it in items[-2:]]
    assert alone == [False, True]
    single_items = {len(items) - 1}

    launches, table_bytes = call_plan(lib, items)
    assert launches is not None
    kinds = [l.kind for l in launches]
    assert kinds == sorted(kinds), "granule launches, tile launches, singles, pixel items"
    assert [(l.format, l.inverse) for l in launches if l.kind == GRANULES] == [(7, 0), (7, 1), (6, 0), (6, 1)]
    tile_keys = [(l.format, l.inverse, l.settings_code) for l in launches if l.kind == TILES]
    assert tile_keys == sorted(set(tile_keys)), "ascending (format, direction, settings code), each once"
    assert [(l.first_item, l.format, l.inverse, l.settings_code) for l in launches if l.kind == SINGLE] == [(len(items) - 1, 1, 0, 0b0101)]

    # every item exactly once: the tile items by their group, the granule items by format and direction, the single, the empty one
    groups = {}
    for i, (it, (fmt, inverse, mode, sa, sc)) in enumerate(zip(items, specs)):
        if it.len and fmt <= 5 and i not in single_items:
            groups.setdefault((fmt, int(inverse), effective_code(fmt, mode, sa, sc)), []).append(it)
    assert tile_keys == sorted(groups)
    assert len(groups) == 10 + 3, "formats 1..5 in both directions, and the second settings of BC1 forward and BC3 in both"
    granule_items = sum(1 for it in items if it.format in (6, 7))
    assert sum(l.items for l in launches) == len(items) - 1 == sum(len(g) for g in groups.values()) + granule_items + len(single_items)
    for l in launches:
        if l.kind != TILES:
            continue
        group = groups[(l.format, l.inverse, l.settings_code)]
        code = l.settings_code
        assert l.items == l.entries == len(group)
        assert l.workgroups == group_alone(lib, l.format, l.inverse, code >> 2, (code >> 1) & 1, code & 1, group)
    check_layout(launches, table_bytes)

    # a pixel item: behind everything when the caller is the host batch, the whole batch refused when it is the device call
    with_pixels = items + [item(lib, 8, False, SRC + (1 << 30), DST + (1 << 30), 999)]
    assert call_plan(lib, with_pixels, 0) == (None, 0)
    more, more_bytes = call_plan(lib, with_pixels, 1)
    assert [(l.kind, l.format, l.first_item) for l in more[len(launches):]] == [(PIXELS, 8, len(items))]
    assert [bytes(a) for a in more[:len(launches)]] == [bytes(b) for b in launches] and more_bytes == table_bytes


def test_settings_are_effective_settings(lib):
    """all 16 settings codes of every format 1..5 in one batch: the groups are those of the format_has_colour /
    format_has_alpha_split arithmetic, which is what settings_code(effective_settings()) must equal"""
    items, want = [], set()
    for fmt in (1, 2, 3, 4, 5):
        for code in range(16):
            mode, sa, sc = code >> 2, (code >> 1) & 1, code & 1
            k = len(items)
            items.append(item(lib, fmt, False, SRC + (k << 20), DST + (k << 20), 300 + k, mode, sa, sc))
            want.add((fmt, 0, effective_code(fmt, mode, sa, sc)))
    launches, _ = call_plan(lib, items)
    assert all(l.kind == TILES for l in launches)
    assert [(l.format, l.inverse, l.settings_code) for l in launches] == sorted(want)
    per_format = {fmt: [l for l in launches if l.format == fmt] for fmt in (1, 2, 3, 4, 5)}
    assert {fmt: len(ls) for fmt, ls in per_format.items()} == {1: 8, 2: 8, 3: 16, 4: 2, 5: 2}
    assert {fmt: sorted(l.items for l in ls) for fmt, ls in per_format.items()} == {1: [2] * 8, 2: [2] * 8, 3: [1] * 16, 4: [8] * 2, 5: [8] * 2}
    # BC4 / BC5: any decorrelation mode and a colour split land in the one group of the alpha split; BC1 / BC2: the alpha split is not seen
    for fmt in (4, 5):
        assert [l.settings_code for l in per_format[fmt]] == [0b0000, 0b0010]
    for fmt in (1, 2):
        assert all(l.settings_code & 0b0010 == 0 for l in per_format[fmt])


@pytest.mark.parametrize("fmt,inverse", [(1, False), (3, False), (3, True), (4, True)])
def test_uniform_and_strided(lib, fmt, inverse):
    tile = 4096 // BLOCK[fmt]   # blocks per tile (256 lanes x 16 bytes; split colours keep BC1 forward at 256 lanes too)
    for tiles in (1, 2, 3):
        blocks, stride_in, stride_out = tiles * tile, 0x10000, 0x24000
        regular = [item(lib, fmt, inverse, SRC + i * stride_in, DST + i * stride_out, blocks) for i in range(4)]
        (l,), _ = call_plan(lib, regular)
        assert (l.workgroups, l.uniform_wgs, l.strided, l.src_stride, l.dst_stride) == (4 * tiles, tiles, 1, stride_in, stride_out)

        moved = list(regular)
        moved[2] = item(lib, fmt, inverse, SRC + 2 * stride_in, DST + 2 * stride_out + 16, blocks)
        (l,), _ = call_plan(lib, moved)
        # (an output 16 bytes on: forward the transformed side leaves its lines and gains an edge tile, so not even uniform)
        assert (l.uniform_wgs, l.strided) == ((tiles, 0) if inverse else (0, 0))
        moved[2] = item(lib, fmt, inverse, SRC + 2 * stride_in + (0 if inverse else 16), DST + 2 * stride_out + (16 if inverse else 0), blocks)
        (l,), _ = call_plan(lib, moved)
        assert (l.workgroups, l.uniform_wgs, l.strided) == (4 * tiles, tiles, 0), "the block side moved by 16 bytes: uniform, not strided"

        longer = list(regular)
        longer[1] = item(lib, fmt, inverse, SRC + stride_in, DST + stride_out, blocks + tile)
        (l,), _ = call_plan(lib, longer)
        assert (l.workgroups, l.uniform_wgs, l.strided) == (4 * tiles + 1, 0, 0)

        (l,), _ = call_plan(lib, regular[:1])
        assert (l.workgroups, l.uniform_wgs, l.strided, l.src_stride, l.dst_stride) == (tiles, tiles, 1, 0, 0)


def granule_plan(lib, items, fmt, inverse):
    arr = array(lib, items)
    n = lib.dxtlt_debug_plan_batch_granules(arr, len(items), fmt, int(inverse), None, None, 0, None, 0)
    first_wg, blocks, coarse = (C.c_uint32 * len(items))(), (C.c_uint64 * len(items))(), (C.c_uint32 * max(1, n))()
    assert lib.dxtlt_debug_plan_batch_granules(arr, len(items), fmt, int(inverse), first_wg, blocks, len(items), coarse, n) == n
    return list(first_wg), list(blocks), list(coarse)[:n]


GRANULE_COUNTS = [1024, 65 * 1024, 3 * 1024 + 5, 7]   # the last is a tail part only


@pytest.mark.parametrize("fmt", [7, 6])
@pytest.mark.parametrize("inverse", [False, True])
def test_granule_plan_and_coarse_index(lib, fmt, inverse):
    items = [item(lib, fmt, inverse, SRC + (k << 24), DST + (k << 24), n) for k, n in enumerate(GRANULE_COUNTS)]
    # (items of the other format and direction do not disturb the plan)
    items.insert(1, item(lib, 13 - fmt, inverse, SRC + (9 << 24), DST + (9 << 24), 2048))
    items.insert(3, item(lib, fmt, not inverse, SRC + (10 << 24), DST + (10 << 24), 5000))
    launches, table_bytes = call_plan(lib, items)
    assert [l.kind for l in launches] == [GRANULES] * 3
    (l,) = [l for l in launches if (l.format, l.inverse) == (fmt, int(inverse))]
    assert (l.items, l.entries, l.tails, l.workgroups) == (4, 3, 2, 69)
    assert l.table_bytes == (32 * (3 + 2) + 4 * 2 + 15) // 16 * 16   # 32-byte entries and tail entries, then the coarse index
    check_layout(launches, table_bytes)

    first_wg, blocks, coarse = granule_plan(lib, items, fmt, inverse)
    assert (first_wg[:3], blocks[:3]) == ([0, 1, 66], [1024, 65 * 1024, 3 * 1024])
    assert len(coarse) == 2 == -(-69 // 64)
    owner_of = [e for e in range(3) for _ in range(blocks[e] // 1024)]
    for w in range(69):
        e = coarse[w // 64]
        assert first_wg[e] <= w - w % 64, "the coarse entry owns the span's first workgroup or starts before it"
        while first_wg[e] + blocks[e] // 1024 <= w:
            e += 1
        assert e == owner_of[w], w


def test_bc7_image_batch_keeps_its_first_workgroups(pkg):
    """the BC7 image batch call builds its coarse index with the same function: the same four buffers, each decoded whole as one
    image, still plan to the first_wg values they always had (and that the plain statement of its plan gives)"""
    lib = load_bc7_image_batch(pkg)
    shapes = {1024: (128, 128), 65 * 1024: (1024, 1040), 3 * 1024 + 5: (68, 724), 7: (28, 4)}
    items = [Bc7ImageItem(n, [(0, *shapes[n])]) for n in GRANULE_COUNTS]
    got = bc7_image_plan(lib, items)
    assert got == bc7_image_plan_of(items)
    assert [(e[4], e[5], e[6]) for e in got] == [(1, 0, -1), (65, 1, -1), (3, 66, 0), (0, 69, 1)]   # granules, first_wg, tail_index
    assert [(e[7], e[8]) for e in got] == [(69, 2)] * 4


def test_table_layout(lib):
    items, _ = mixed_batch(lib)
    launches, table_bytes = call_plan(lib, items)
    check_layout(launches, table_bytes)
    tables = [l for l in launches if l.kind in (GRANULES, TILES)]
    assert len(tables) == 4 + 13 and tables[-1].table_offset + tables[-1].table_bytes == table_bytes
    for l in tables:
        if l.kind == TILES:   # 96-byte entries, then base[ceil(wgs / 4096)] and two bytes of room per 64 workgroups, padded to 16
            index = (4 * -(-l.workgroups // 4096) + 2 * -(-l.workgroups // 64) + 15) // 16 * 16
            assert l.table_bytes == 96 * l.entries + index
    # nothing is left after filtering: no launch, no byte
    assert call_plan(lib, []) == ([], 0)
    assert call_plan(lib, [item(lib, f, inv, 0, 0, 0) for f in range(1, 8) for inv in (0, 1)]) == ([], 0)
    assert call_plan(lib, [item(lib, 8, False, 0, 0, 0)], 1) == ([], 0)
    # singles and pixel items have no table
    only_alone = [item(lib, 1, False, SRC, DST + 2, 1000), item(lib, 9, True, SRC + (1 << 20), DST + (1 << 20), 10)]
    launches, table_bytes = call_plan(lib, only_alone, 1)
    assert [l.kind for l in launches] == [SINGLE, PIXELS] and table_bytes == 0


def defects(lib):
    """(name, the defective item, takes it the device call / the host call's validation?, status, text of the device call, of the
    host call) for every check of the two validation loops.  A defect sits behind sound items: a batch is refused whole."""
    big = 1 << 32
    return [
        ("format 0", lib.Item(SRC, DST, 16, 0, 0, 1, 1, 1), E_ARGUMENT, "format must be 1..5 (BC1..BC5), 6 (BC6H) or 7", "8 (4-byte pixels) or 9"),
        ("format 10", lib.Item(SRC, DST, 16, 10, 0, 1, 1, 1), E_ARGUMENT, "format must be 1..5 (BC1..BC5), 6 (BC6H) or 7", "8 (4-byte pixels) or 9"),
        ("length", lib.Item(SRC, DST, 24, 3, 0, 1, 1, 1), E_LENGTH, "len is not a multiple", "len is not a multiple"),
        ("mode", lib.Item(SRC, DST, 32, 2, 1, 4, 1, 1), E_ARGUMENT, "decorrelation_mode must be 0..3", "decorrelation_mode must be 0..3"),
        ("NULL input", lib.Item(None, DST, 32, 7, 0, 0, 0, 0), E_ARGUMENT, "NULL device buffer with len > 0", "NULL buffer with len > 0"),
        ("NULL output", lib.Item(SRC, None, 8, 4, 1, 0, 0, 0), E_ARGUMENT, "NULL device buffer with len > 0", "NULL buffer with len > 0"),
        ("host: 4 GiB", lib.Item(SRC, DST, big, 1, 0, 1, 1, 1), None, None, "4 GiB or more"),
        ("host: pixels overlap", lib.Item(SRC, SRC + 8, 16, 8, 0, 1, 1, 1), E_ARGUMENT, "format must be 1..5", "pixel input and output overlap"),
    ]


def test_a_defective_batch_is_refused_whole(lib):
    sound = [item(lib, 1, False, SRC, DST, 512), item(lib, 7, True, SRC + (1 << 20), DST + (1 << 20), 2048)]
    assert call_plan(lib, sound)[0] is not None
    for name, bad, status, device_text, host_text in defects(lib):
        arr = array(lib, sound + [bad])
        if status is not None:
            assert call_plan(lib, sound + [bad]) == (None, 0), name
            assert lib.dxtlt_transform_batch_device(arr, 3, None) == status, name
            assert device_text in lib.dxtlt_last_error().decode(), name
        # (the host call checks everything before it touches a device or a buffer)
        assert lib.dxtlt_transform_batch_host(arr, 3) == (E_ARGUMENT if status is None else status), name
        assert host_text in lib.dxtlt_last_error().decode(), name
    # what the format ignores is not checked: a BC4 item with a decorrelation mode of 9 is planned, a BC7 item with one too
    assert call_plan(lib, sound + [lib.Item(SRC, DST, 8, 4, 0, 9, 1, 1), lib.Item(SRC, DST, 16, 7, 0, 9, 1, 1)])[0] is not None
    # the pixel overlap is a defect of the device batch too when pixel items are allowed; a NULL pointer with len == 0 is none
    overlap = lib.Item(SRC, SRC + 8, 16, 8, 0, 1, 1, 1)
    assert call_plan(lib, sound + [overlap], 1) == (None, 0)
    assert call_plan(lib, sound + [lib.Item(None, None, 0, 3, 0, 1, 1, 1)])[0] is not None
    assert lib.dxtlt_debug_plan_batch_call(None, 3, 0, None, 0, None) == -1
    assert lib.dxtlt_transform_batch_device(None, 3, None) == E_ARGUMENT


def test_launch_limits(lib):
    """one launch holds at most 0xFFFFFF workgroups; addresses are numbers, so the sizes cost nothing"""
    # tiles: 0xFFFFFF tiles of BC3 (just under 64 GiB) fill a launch, one more tile in the same group is too much -- and fits when
    # it is another group's; an item of 64 GiB is refused by itself
    full = item(lib, 3, False, SRC, DST, MAX_WGS * 256)
    (l,), _ = call_plan(lib, [full])
    assert (l.workgroups, l.uniform_wgs, l.strided) == (MAX_WGS, MAX_WGS, 1)
    one_more = item(lib, 3, False, SRC + (1 << 40), DST + (1 << 40), 256)
    arr = array(lib, [full, one_more])
    assert call_plan(lib, [full, one_more]) == (None, 0)
    assert lib.dxtlt_transform_batch_device(arr, 2, None) == E_ARGUMENT
    assert "64 GiB or more of one format, direction and settings" in lib.dxtlt_last_error().decode()
    assert len(call_plan(lib, [full, item(lib, 3, True, SRC + (1 << 40), DST + (1 << 40), 256)])[0]) == 2
    arr = array(lib, [one_more, item(lib, 2, False, SRC, DST, 1 << 32)])
    assert lib.dxtlt_debug_plan_batch_call(arr, 2, 0, None, 0, None) == -1
    assert lib.dxtlt_transform_batch_device(arr, 2, None) == E_ARGUMENT
    assert "batch item of 64 GiB or more" in lib.dxtlt_last_error().decode()
    # granules: 0xFFFFFF of one format and direction fill a launch, over several items too
    for fmt, name in ((7, "BC7"), (6, "BC6H")):
        parts = [item(lib, fmt, True, SRC, DST, (MAX_WGS - 5) * 1024 + 3), item(lib, fmt, True, SRC + (1 << 42), DST + (1 << 42), 5 * 1024)]
        (l,), _ = call_plan(lib, parts)
        assert (l.workgroups, l.entries, l.tails) == (MAX_WGS, 2, 1)
        one_granule = item(lib, fmt, True, SRC + (1 << 43), DST + (1 << 43), 1024)
        assert call_plan(lib, parts + [one_granule]) == (None, 0)
        assert lib.dxtlt_transform_batch_device(array(lib, parts + [one_granule]), 3, None) == E_ARGUMENT
        assert f"256 GiB or more of {name} in one direction" in lib.dxtlt_last_error().decode()
        assert len(call_plan(lib, parts + [item(lib, fmt, False, SRC + (1 << 43), DST + (1 << 43), 1024)])[0]) == 2
