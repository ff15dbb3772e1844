"""The planners of the batched pixel calls without a device (csrc/pixel_batch_plan.h through dxtlt_debug_plan_pixels_batch and
dxtlt_debug_plan_pixels_batch_auto: addresses are numbers, nothing is dereferenced): classes, entries, the workgroup index's form,
every refusal with its status, arena slices, sections, counters and chunks -- and a count of what the case lists of
tests/test_pixels_batch_gpu.py reach."""
import ctypes as C

import pytest

import pixels_batch_util as U

OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
A, B_ = 0x10_0000_0000, 0x20_0000_0000       # two made-up address ranges far apart


@pytest.fixture(scope="module")
def lib(pkg):
    return U.load(pkg)


def items_of(specs):
    """specs: (d_input, d_output, len, pixel_bytes, inverse, decorrelate, layout)"""
    arr = (U.Item * max(1, len(specs)))()
    for k, s in enumerate(specs):
        arr[k].d_input, arr[k].d_output, arr[k].len, arr[k].pixel_bytes, arr[k].inverse, arr[k].decorrelate, arr[k].layout = s
    return arr


def auto_items_of(specs):
    """specs: (d_input, d_output, len, pixel_bytes)"""
    arr = (U.AutoItem * max(1, len(specs)))()
    for k, s in enumerate(specs):
        arr[k].d_input, arr[k].d_output, arr[k].len, arr[k].pixel_bytes = s
        arr[k].decorrelate, arr[k].layout = 0xEE, 0xEE
    return arr


def auto_plan(lib, specs, chunk_capacity=64):
    arr = auto_items_of(specs)
    items = (U.PlanItem * max(1, len(specs)))()
    chunks = (U.PlanChunk * chunk_capacity)()
    n = C.c_size_t(123)
    rc = lib.dxtlt_debug_plan_pixels_batch_auto(arr, len(specs), items, chunks, chunk_capacity, C.byref(n))
    return rc, list(items[:len(specs)]), list(chunks[:min(n.value, chunk_capacity)]), n.value


# ---- the manual batch ------------------------------------------------------------------------------------------------------------
def test_one_record_per_class_present_in_stream_order(lib):
    cases = U.cases_every_class()
    n, launches, table_bytes = U.plan(lib, U.fake_items(cases), len(cases))
    assert n == 24 == len(launches)
    assert [(l.pixel_bytes, l.inverse, l.decorrelate, l.layout) for l in launches] == U.CLASSES
    at = 0
    for l in launches:
        mine = [c for c in cases if c[1:5] == (l.pixel_bytes, l.inverse, l.decorrelate, l.layout)]
        assert l.items == 2 == len(mine) and l.workgroups == sum(-(-c[0] // U.TILE) for c in mine) and l.wide == 0
        assert l.table_offset == at and l.table_offset % 16 == 0 and l.table_bytes % 16 == 0
        base, delta = -(-l.workgroups // 4096), -(-l.workgroups // 64)
        assert l.table_bytes == 32 * l.items + ((4 * base + 2 * delta + 15) & ~15)
        at += l.table_bytes
    assert table_bytes == at
    assert sum(l.items for l in launches) == len(cases)
    # records beyond the capacity are counted, not written
    assert U.plan(lib, U.fake_items(cases), len(cases), cap=3)[0] == 24
    # a mixed batch of three classes, a decorrelate flag that is not 1
    specs = [(A, B_, 4096 * 4, 4, 0, 7, 2), (A + 0x100000, B_ + 0x100000, 12, 4, 0, 1, 2), (A, B_ + 0x200000, 9, 3, 1, 0, 0),
             (A, B_ + 0x300000, 3, 3, 0, 0, 0)]
    n, launches, _ = U.plan(lib, items_of(specs), len(specs))
    assert [(l.pixel_bytes, l.inverse, l.decorrelate, l.layout, l.items, l.workgroups) for l in launches] == \
        [(4, 0, 1, 2, 2, 2), (3, 0, 0, 0, 1, 1), (3, 1, 0, 0, 1, 1)]


def test_the_wide_index_and_empty_items(lib):
    one_tile = [(A + 0x10000 * k, B_ + 0x10000 * k, 4 * 100, 4, 0, 1, 2) for k in range(300)]
    n, launches, _ = U.plan(lib, items_of(one_tile), 300)
    assert n == 1 and (launches[0].items, launches[0].workgroups, launches[0].wide) == (300, 300, 1)     # 300 entries begin in one span
    n, launches, _ = U.plan(lib, items_of(one_tile[:255]), 255)
    assert n == 1 and launches[0].wide == 0
    cases = U.cases_wide_lookup()
    n, launches, _ = U.plan(lib, U.fake_items(cases), len(cases))
    assert n == 1 and launches[0].wide == 1 and launches[0].items == 300
    # empty items own nothing: no entry, no workgroup, no launch, and they need no pointers
    empty = (0, 0, 0, 4, 0, 1, 2)
    n, launches, table_bytes = U.plan(lib, items_of([empty, one_tile[0], empty, (0, 0, 0, 3, 1, 0, 0)]), 4)
    assert n == 1 and (launches[0].items, launches[0].workgroups) == (1, 1)
    assert U.plan(lib, items_of([empty, empty]), 2) == (0, [], 0)
    assert U.plan(lib, None, 0) == (0, [], 0)
    assert lib.dxtlt_transform_pixels_batch_device(None, 0, None) == OK
    assert lib.dxtlt_transform_pixels_batch_device(items_of([empty, empty]), 2, None) == OK           # nothing to enqueue: no device needed


REFUSALS = [
    ("pixel_bytes", (A, B_, 8, 2, 0, 1, 2), E_ARGUMENT), ("pixel_bytes", (A, B_, 10, 5, 0, 1, 2), E_ARGUMENT),
    ("pixel_bytes", (0, 0, 0, 0, 0, 1, 2), E_ARGUMENT),                        # checked on empty items too
    ("layout", (A, B_, 8, 4, 0, 1, 3), E_ARGUMENT), ("layout", (A, B_, 9, 3, 1, 0, 255), E_ARGUMENT),
    ("NULL", (0, B_, 8, 4, 0, 1, 2), E_ARGUMENT), ("NULL", (A, 0, 8, 4, 1, 1, 2), E_ARGUMENT),
    ("multiple", (A, B_, 10, 4, 0, 1, 2), E_LENGTH), ("multiple", (A, B_, 10, 3, 0, 1, 2), E_LENGTH),
    ("64 GiB", (A, B_, 64 << 30, 4, 0, 1, 2), E_ARGUMENT),
    ("overlaps", (A, A + 4, 8, 4, 0, 1, 2), E_ARGUMENT),                       # an output over its own input
]


@pytest.mark.parametrize("what, bad, status", REFUSALS)
def test_every_refusal_has_its_status_wherever_the_item_stands(lib, what, bad, status):
    ok = (A + (1 << 32), B_ + (1 << 32), 4096 * 4, 4, 0, 1, 2)
    for specs in ([bad], [ok, bad], [bad, ok]):
        arr = items_of(specs)
        assert U.plan(lib, arr, len(specs))[0] == -1, what
        assert what.encode() in lib.dxtlt_last_error(), lib.dxtlt_last_error()
        assert lib.dxtlt_transform_pixels_batch_device(arr, len(specs), None) == status, what          # before any device work
    auto = auto_items_of([bad[:4]])
    if what != "layout":
        assert lib.dxtlt_transform_pixels_batch_auto_device(auto, 1, None) == status
        assert auto_plan(lib, [bad[:4]])[0] == status
        assert (auto[0].decorrelate, auto[0].layout) == (0xEE, 0xEE)                                    # results untouched


def test_null_items_and_the_launch_limit(lib):
    assert lib.dxtlt_transform_pixels_batch_device(None, 3, None) == E_ARGUMENT
    assert lib.dxtlt_debug_plan_pixels_batch(None, 3, None, 0, None) == -1
    assert lib.dxtlt_transform_pixels_batch_auto_device(None, 3, None) == E_ARGUMENT
    assert lib.dxtlt_debug_plan_pixels_batch_auto(None, 3, None, None, 0, None) == E_ARGUMENT
    # one launch holds fewer than 2^24 tiles: five items of 63 GiB of 4-byte pixels are 20.6 million tiles of one class; four are
    # fine, and so are five in two classes
    big = [((k + 1) << 40, ((k + 1) << 40) + (1 << 39), 63 << 30, 4, 0, 1, 2) for k in range(5)]
    assert U.plan(lib, items_of(big), 5)[0] == -1 and b"one launch" in lib.dxtlt_last_error()
    assert lib.dxtlt_transform_pixels_batch_device(items_of(big), 5, None) == E_ARGUMENT
    n, launches, _ = U.plan(lib, items_of(big[:4]), 4)
    assert n == 1 and launches[0].workgroups == 4 * (63 << 30) // 16384 < (1 << 24)
    split = big[:3] + [b[:4] + (1,) + b[5:] for b in big[3:]]
    assert U.plan(lib, items_of(split), 5)[0] == 2
    # the auto call holds all items of one pixel_bytes to the limit together, whichever settings would win
    assert auto_plan(lib, [b[:4] for b in big])[0] == E_ARGUMENT
    assert auto_plan(lib, [b[:4] for b in big[:4]])[0] == OK
    mixed = [b[:4] for b in big[:3]] + [(b[0], b[1], 63 << 30, 3) for b in big[3:]]
    assert auto_plan(lib, mixed)[0] == OK


def test_an_output_overlaps_nothing_but_inputs_may_overlap(lib):
    n = 4096
    ok = (A, B_, n, 4, 0, 1, 2)
    for other in [(A + 0x100000, B_ + n - 1, n, 4, 0, 1, 2),       # two outputs, one byte shared
                  (A + 0x100000, B_ - n + 1, n, 4, 0, 1, 2),
                  (A + 0x100000, A + n - 1, n, 4, 1, 0, 0),         # an output over another item's input
                  (B_ + n - 4, A + 0x100000, n, 4, 1, 0, 0)]:       # an input over another item's output
        for specs in ([ok, other], [other, ok]):                    # in both orders
            assert U.plan(lib, items_of(specs), 2)[0] == -1, other
            assert b"overlaps" in lib.dxtlt_last_error()
            assert auto_plan(lib, [s[:4] for s in specs])[0] == E_ARGUMENT
    for other in [(A, B_ + n, n, 4, 0, 1, 2),                       # the same input, outputs side by side
                  (A + 8, B_ - n, n, 4, 1, 1, 2),                   # inputs that overlap
                  (A + n, B_ + 2 * n, n, 3 + 1, 0, 0, 0)]:
        for specs in ([ok, other], [other, ok]):
            assert U.plan(lib, items_of(specs), 2)[0] >= 1, other
            assert auto_plan(lib, [s[:4] for s in specs])[0] == OK


# ---- the auto batch --------------------------------------------------------------------------------------------------------------
def auto_specs():
    lens = [0, 4, 3 * 17, 4 * 4097, 3 * (32768 + 7), 4 * 87381, 0, 3 * 87381, 4 * 8191]
    return [(A + (k << 24) + k, B_ + (k << 24) + 3 * k, n, 4 if n % 4 == 0 and k != 7 else 3) for k, n in enumerate(lens)]


def check_auto_plan(specs, items, chunks):
    for k, ((_i, _o, n, _B), it) in enumerate(zip(specs, items)):
        assert it.arena_offset % 16 == 0 and it.arena_bytes == 5 * n, k
        for i, s in enumerate(it.sections):
            assert s.len == n and s.counter == 6 * k + i, (k, i)
            assert (s.in_arena, s.offset) == ((1, it.arena_offset + i * n) if i < 5 else (0, 0)), (k, i)
    at = 0
    for c, ch in enumerate(chunks):
        assert ch.first_item == at and ch.item_count >= 1, c
        mine = list(range(at, at + ch.item_count))
        at += ch.item_count
        assert all(items[i].chunk == c for i in mine)
        spans = sorted((items[i].arena_offset, items[i].arena_offset + items[i].arena_bytes) for i in mine)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), c       # slices disjoint within the chunk
        assert spans[-1][1] <= ch.arena_bytes
        assert ch.estimator_workgroups == sum(6 * -(-specs[i][2] // U.WINDOW) for i in mine), c
        assert ch.candidate_launches == len({specs[i][3] for i in mine if specs[i][2]}), c
    assert at == len(items)


def test_auto_slices_sections_counters_and_chunks(lib):
    specs = auto_specs()
    rc, items, chunks, n = auto_plan(lib, specs)
    assert rc == OK and n == 1 == len(chunks) and chunks[0].candidate_launches == 2
    check_auto_plan(specs, items, chunks)
    cap = 5 * 4 * 8191 + 5 * 3 * (32768 + 7) + 64           # two of the mid-sized items at the most; the two chains are larger
    lib.dxtlt_debug_batch_auto_arena_cap(cap)
    try:
        rc, small, small_chunks, n = auto_plan(lib, specs)
        counted = auto_plan(lib, specs, chunk_capacity=2)
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)
    assert rc == OK and n == len(small_chunks) >= 4
    assert counted[0] == OK and counted[3] == n and len(counted[2]) == 2         # counted, not written
    check_auto_plan(specs, small, small_chunks)
    oversize = [i for i, it in enumerate(small) if it.arena_bytes > cap]
    assert len(oversize) == 2
    for i in oversize:
        assert small_chunks[small[i].chunk].item_count == 1, i                   # alone in its chunk
    for ch in small_chunks:
        assert ch.arena_bytes <= cap or ch.item_count == 1
    for a, b in zip(small_chunks, small_chunks[1:]):                             # a chunk is closed only when the next item would not fit
        assert a.arena_bytes + ((small[b.first_item].arena_bytes + 15) & ~15) > cap
    for a, b in zip(items, small):                                               # sections and counters do not depend on the cap
        assert [(s.len, s.counter) for s in a.sections] == [(s.len, s.counter) for s in b.sections]
    assert auto_plan(lib, specs)[3] == 1                                         # the hook is back at 0: the default cap


def test_an_all_empty_auto_batch_keeps_the_first_candidate_without_a_device(lib):
    arr = auto_items_of([(0, 0, 0, 4), (0, 0, 0, 3)])
    assert lib.dxtlt_transform_pixels_batch_auto_device(arr, 2, None) == OK
    assert [(a.decorrelate, a.layout) for a in arr] == [(1, 2), (1, 2)]
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    lib.dxtlt_debug_pixels_batch_auto_last(out)
    assert list(out) == [0, 0, 0, 0]
    assert lib.dxtlt_debug_pixels_batch_auto_last_totals(0, None, 0) == 0
    assert lib.dxtlt_transform_pixels_batch_auto_device(None, 0, None) == OK


# ---- what the case lists of the GPU tests reach, by exact count ---------------------------------------------------------------------
def test_the_gpu_case_lists_reach_what_they_claim(lib):
    every = U.cases_every_class()
    assert sorted({c[1:5] for c in every}) == sorted(U.CLASSES) and len(every) == 48
    assert {c[0] for c in every} == set(U.COUNTS)
    # both index forms, and in each the entry that the index names (direct) and the bisection behind it
    wide = U.cases_wide_lookup()
    assert U.plan(lib, U.fake_items(wide), len(wide))[1][0].wide == 1
    (direct, bisected), = U.lookup_arms(wide).values()
    # 42 rounds of 1, 1, 2, 2, 3, 3, 3 tiles and 1, 1, 2, 2, 3, 3: 642 workgroups in 11 groups of 64, in each of which only the first
    # entry's one to three workgroups are named by the index
    assert direct + bisected == sum(-(-c[0] // U.TILE) for c in wide) == 642 and (direct, bisected) == (21, 621)
    long_ = U.cases_long_entries()
    launch, = U.plan(lib, U.fake_items(long_), len(long_))[1]
    assert launch.wide == 0 and launch.workgroups == 1 + 64 + 1 + 65 + 1 + 130 + 1 == 263
    (direct, bisected), = U.lookup_arms(long_).values()
    # entries end at 1, 65, 66, 131, 132, 262, 263: the groups of 64 begin in entries 0, 1, 3, 5, 5, which own 1, 1 (workgroup 64), 3
    # (128..130), 64 and 6 (256..261) of their group's workgroups
    assert (direct, bisected) == (1 + 1 + 3 + 64 + 6, 263 - 75)
    assert [-(-c[0] // U.TILE) for c in long_] == [1, 64, 1, 65, 1, 130, 1]
    assert long_[3][0] % U.TILE == U.TILE - 1 and long_[5][0] % U.TILE == 1      # a last tile one pixel short, a last tile of one pixel
    for n in (1, 2, 64, 65):
        launch, = U.plan(lib, U.fake_items(U.cases_count(n)), n)[1]
        assert (launch.items, launch.workgroups) == (n, 2 * n)
    # every residue of a 128-byte line on both sides, in every direction and pixel size
    for B in (3, 4):
        for inverse in (0, 1):
            cases = U.cases_alignment(B, inverse)
            assert sorted(c[5] for c in cases) == list(range(128)) == sorted(c[6] for c in cases)
            assert all(c[0] == 4097 and c[1:5] == (B, inverse, 1, 2) for c in cases)
            arr = U.fake_items(cases)
            assert [arr[k].d_input % 128 for k in range(128)] == [c[5] for c in cases]
            assert [arr[k].d_output % 128 for k in range(128)] == [c[6] for c in cases]
            assert U.plan(lib, arr, 128)[0] == 1
    mix = U.cases_mix()
    assert len(mix) == 40 and sorted({c[1:5] for c in mix}) == sorted(U.CLASSES)
    assert U.plan(lib, U.fake_items(mix), 40)[0] == 24
