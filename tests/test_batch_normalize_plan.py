"""What dxtlt_transform_batch_with_normalize_blocks_device enqueues for a whole batch, checked without a GPU through
dxtlt_debug_plan_batch_normalize_call (include/dxtlt_batch_normalize.h): the hook runs the call's own planner and table writer
(plan_batch_normalize, csrc/batch_normalize_api.cpp) on addresses that are only numbers.

1. A batch of all three formats with every colour mode and all 12 BC3 mode pairs over two settings codes: one plain launch per
   (format, settings) that has all-None items, ONE normalising launch per (format, settings) for BC2 / BC3 whatever the modes, one
   per (settings, colour mode) for BC1, in ascending (format, settings code, plain before normalising, BC1 mode); items, entries and
   workgroups add up to the batch; the tables tile the staged buffer.
2. An item whose d_output is off an 8-byte boundary goes out alone (kind 2), behind the tile launches.
3. A batch with every mode None plans exactly as dxtlt_debug_plan_batch_call plans the same items, field for field.
4. Every defect is refused with its status, in the documented order; a defective item refuses the batch whole.
5. count == 0 plans nothing."""
import ctypes as C

import pytest

from batch_normalize_common import (ALL_OFF, BLOCK, DEFAULT, E_ARGUMENT, E_LENGTH, FMT_ID, FORMATS, MODE_PAIRS, NORMALIZING, PLAIN, SINGLE, Item,
                                    array, bind, item, settings_code, tile_blocks)
from test_batch_call_plan import call_plan as plain_call_plan, lib as plain_lib  # noqa: F401

SRC, DST = 0x7F00_0000_0000, 0x7E00_0000_0000   # made-up device addresses on 4 KiB pages
MAX_WGS = 0xFFFFFF


@pytest.fixture(scope="module")
def lib(pkg):
    return bind(pkg)


def plan(lib, items):
    """(the launches, the staged buffer's bytes), or (minus the status, 0) for a batch the call refuses"""
    arr, nbytes = array(items), C.c_uint64(99)
    n = lib.dxtlt_debug_plan_batch_normalize_call(arr, len(items), None, 0, C.byref(nbytes))
    if n < 0:
        assert nbytes.value == 0
        return n, 0
    out = (lib.Launch * max(1, n))()
    assert lib.dxtlt_debug_plan_batch_normalize_call(arr, len(items), out, n, C.byref(nbytes)) == n
    return list(out)[:n], nbytes.value


def wgs_of(fmt, s, blocks, aligned):
    """workgroups of an item whose transformed side starts on a 4 KiB page: whole tiles and an edge tile for the rest -- and, when
    the streams do not all start on 128-byte lines (halo form), for the stream tails"""
    T = tile_blocks(fmt, s)
    return blocks // T + (1 if blocks % T or not aligned else 0)


def mixed_batch():
    """(fmt, settings, modes, blocks) of every item: per format and settings (default, all off) every mode pair -- None too -- at
    sizes that change from item to item"""
    out = []
    for fmt in FORMATS:
        for s in (DEFAULT[fmt], ALL_OFF):
            for k, modes in enumerate([(0, 0)] + MODE_PAIRS[fmt] + [(0, 0)]):
                out.append((fmt, s, modes, 100 + 300 * k + 7 * len(out)))
    return out


def items_of(batch):
    items, at = [], 0
    for fmt, s, modes, blocks in batch:
        n = blocks * BLOCK[fmt]
        items.append(item(fmt, SRC + at, DST + at, n, modes, s))
        at += (n + 4095) & ~4095
    return items


def test_one_launch_per_group_in_ascending_order(lib):
    batch = mixed_batch()
    assert {m for f, _, m, _ in batch if f == "bc3"} == {(a, c) for a in range(4) for c in range(3)}
    launches, table_bytes = plan(lib, items_of(batch))
    want = []
    for fmt in FORMATS:
        for s in sorted({DEFAULT[fmt], ALL_OFF}, key=lambda s: settings_code(fmt, s)):
            code = settings_code(fmt, s)
            mine = [(m, b) for f, t, m, b in batch if f == fmt and t == s]
            want.append((PLAIN, FMT_ID[fmt], code, [b for m, b in mine if m == (0, 0)]))
            if fmt == "bc1":
                for c in (1, 2):
                    want.append((NORMALIZING, 1, code | c << 8, [b for m, b in mine if m[1] == c]))
            else:
                want.append((NORMALIZING, FMT_ID[fmt], code, [b for m, b in mine if m != (0, 0)]))
    assert [(l.kind, l.format, l.settings_code, l.items) for l in launches] == [(k, f, c, len(b)) for k, f, c, b in want]
    assert all(len(b) > 0 for _, _, _, b in want) and len(launches) == 2 * 3 + 2 * 2 + 2 * 2
    # ascending key: format, settings code, plain before normalising, BC1 colour mode
    keys = [(l.format, l.settings_code & 15, l.kind, l.settings_code >> 8) for l in launches]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(l.inverse == 0 and l.entries == l.items and l.tails == 0 for l in launches)
    assert all(l.strided == 0 for l in launches if l.kind == NORMALIZING)
    assert sum(l.items for l in launches) == sum(l.entries for l in launches) == len(batch)
    # page-aligned outputs of odd sizes: every stream but the first starts off a 128-byte line, so every item is in halo form
    assert sum(l.workgroups for l in launches) == sum(wgs_of(f, s, b, False) for f, s, _, b in batch)
    at = 0
    for l in launches:
        assert l.table_offset == at and l.table_offset % 16 == 0 and l.table_bytes % 16 == 0 and l.table_bytes >= 96 * l.entries
        at += l.table_bytes
    assert at == table_bytes


def test_mixed_modes_of_bc3_share_one_launch_with_uniform_sizes(lib):
    """eleven BC3 items of one size, one per mode pair: one normalising launch that divides instead of looking up"""
    s, n = DEFAULT["bc3"], 257
    launches, _ = plan(lib, items_of([("bc3", s, m, n) for m in MODE_PAIRS["bc3"]]))
    assert len(launches) == 1
    l = launches[0]
    assert (l.kind, l.format, l.settings_code, l.items, l.uniform_wgs, l.workgroups, l.strided) == (NORMALIZING, 3, settings_code("bc3", s), 11, 2, 22, 0)


def test_an_output_off_its_element_width_goes_out_alone(lib):
    s = DEFAULT["bc3"]
    items = items_of([("bc3", s, (3, 2), 300), ("bc3", s, (1, 1), 300), ("bc1", DEFAULT["bc1"], (0, 2), 700), ("bc2", ALL_OFF, (0, 0), 300)])
    for k in (1, 2, 3):
        items[k].d_output += 1                      # colour endpoints (2 or 4 bytes each) at an odd address
    launches, _ = plan(lib, items)
    assert [(l.kind, l.format, l.first_item) for l in launches if l.kind == SINGLE] == [(SINGLE, 3, 1), (SINGLE, 1, 2), (SINGLE, 2, 3)]
    assert [l.kind for l in launches] == [NORMALIZING, SINGLE, SINGLE, SINGLE]
    assert [l.settings_code for l in launches[1:]] == [settings_code("bc3", s), settings_code("bc1", DEFAULT["bc1"]), settings_code("bc2", ALL_OFF)]
    assert all(l.items == 1 and l.workgroups == 0 for l in launches[1:])


def test_all_none_batches_plan_as_the_plain_batch_call_does(lib, plain_lib):
    batch = [(f, s, (0, 0), b) for f, s, _, b in mixed_batch()] + [("bc2", DEFAULT["bc2"], (0, 0), 512)] * 3
    items = items_of(batch)
    items[-1].alpha_mode = 3                       # ignored on BC2: still all None
    plain = [plain_lib.Item(it.d_input, it.d_output, it.len, it.format, 0, it.decorrelation_mode, it.split_alpha_endpoints,
                            it.split_colour_endpoints) for it in items]
    plain[3].d_output = items[3].d_output = items[3].d_output + 1          # one single among them
    mine, my_bytes = plan(lib, items)
    theirs, their_bytes = plain_call_plan(plain_lib, plain)
    assert my_bytes == their_bytes and len(mine) == len(theirs) > 6
    fields = [name for name, _ in lib.Launch._fields_]
    assert [[getattr(l, f) for f in fields] for l in mine] == [[getattr(l, f) for f in fields] for l in theirs]
    assert {l.kind for l in mine} == {PLAIN, SINGLE}


def good(fmt="bc3", blocks=300, modes=(1, 1)):
    return item(fmt, SRC, DST, blocks * BLOCK[fmt], modes, DEFAULT[fmt])


def broken(**fields):
    it = good(fields.pop("fmt", "bc3"))
    for k, v in fields.items():
        setattr(it, k, v)
    return it


DEFECTS = [   # in the order in which the call reports them: (item, status, a word of the message)
    (broken(format=0), E_ARGUMENT, "format"),
    (broken(format=4), E_ARGUMENT, "format"),
    (broken(len=300 * 16 + 8), E_LENGTH, "multiple"),
    (broken(fmt="bc1", len=300 * 8 + 4), E_LENGTH, "multiple"),
    (broken(decorrelation_mode=4), E_ARGUMENT, "decorrelation_mode"),
    (broken(color_mode=3), E_ARGUMENT, "color_mode"),
    (broken(fmt="bc1", color_mode=3), E_ARGUMENT, "color_mode"),
    (broken(alpha_mode=4), E_ARGUMENT, "alpha_mode"),
    (broken(d_input=0), E_ARGUMENT, "NULL"),
    (broken(d_output=0), E_ARGUMENT, "NULL"),
    (broken(len=64 << 30), E_ARGUMENT, "64 GiB"),
]


@pytest.mark.parametrize("k", range(len(DEFECTS)))
def test_every_defect_is_refused_with_its_status(lib, k):
    bad, status, word = DEFECTS[k]
    for items in ([bad], [good(), good("bc1"), bad], [bad, good()]):
        assert plan(lib, items) == (-status, 0)
        assert word in lib.dxtlt_last_error().decode()
        assert lib.dxtlt_transform_batch_with_normalize_blocks_device(array(items), len(items), None) == status   # before any device work


def test_defects_are_reported_in_the_documented_order(lib):
    """an item with every defect at once loses them one by one, in the order of the header"""
    it = broken(format=9, len=300 * 16 + 8, decorrelation_mode=7, color_mode=5, alpha_mode=9, d_input=0)
    seen = []
    for fix in (dict(format=3), dict(len=300 * 16), dict(decorrelation_mode=1), dict(color_mode=2), dict(alpha_mode=3), dict(d_input=SRC)):
        status, _ = plan(lib, [it])
        seen.append((status, lib.dxtlt_last_error().decode()))
        for k, v in fix.items():
            setattr(it, k, v)
    assert [s for s, _ in seen] == [-E_ARGUMENT, -E_LENGTH, -E_ARGUMENT, -E_ARGUMENT, -E_ARGUMENT, -E_ARGUMENT]
    for (_, text), word in zip(seen, ("format", "multiple", "decorrelation_mode", "color_mode", "alpha_mode", "NULL")):
        assert word in text
    assert plan(lib, [it])[0][0].kind == NORMALIZING
    # what BC1 / BC2 ignore is no defect; an empty item needs no buffer; reserved bytes are ignored
    ok = [broken(fmt="bc1", alpha_mode=200), broken(fmt="bc2", alpha_mode=200), broken(len=0, d_input=0, d_output=0)]
    ok[0].reserved[0] = ok[0].reserved[1] = 0xFF
    launches, _ = plan(lib, ok)
    assert [(l.kind, l.format, l.items) for l in launches] == [(NORMALIZING, 1, 1), (NORMALIZING, 2, 1)]


def test_a_launch_of_2_to_the_24_workgroups_is_refused(lib):
    """a launch holds fewer than 2^32 threads: 2^24 - 1 workgroups of 256 lanes"""
    per_item = (32 << 30) // 16                      # blocks of a 32 GiB BC3 item: 2^23 tiles (+ 1 edge tile for the stream tails)
    a, b = good(blocks=per_item), good(blocks=per_item, modes=(2, 0))
    b.d_input, b.d_output = SRC + (1 << 40), DST + (1 << 40)
    assert plan(lib, [a, b]) == (-E_ARGUMENT, 0) and "too large" in lib.dxtlt_last_error().decode()
    launches, _ = plan(lib, [a])
    assert launches[0].workgroups <= MAX_WGS
    # a plain item beside it is another launch
    c = good(blocks=per_item, modes=(0, 0))
    c.d_input, c.d_output = b.d_input, b.d_output
    assert [l.kind for l in plan(lib, [a, c])[0]] == [PLAIN, NORMALIZING]


def test_an_empty_batch_plans_nothing(lib):
    assert plan(lib, []) == ([], 0)
    assert lib.dxtlt_debug_plan_batch_normalize_call(None, 0, None, 0, None) == 0
    assert lib.dxtlt_transform_batch_with_normalize_blocks_device(None, 0, None) == 0
    assert plan(lib, [broken(len=0), broken(fmt="bc1", len=0)]) == ([], 0)
    assert lib.dxtlt_debug_plan_batch_normalize_call(None, 3, None, 0, None) == -E_ARGUMENT
