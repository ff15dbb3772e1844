"""The host planner of dxtlt_transform_batch_auto_device without a device (dxtlt_debug_plan_batch_auto: addresses are numbers,
nothing is dereferenced): arena slices, sections, counters, estimator workgroups and chunks."""
import ctypes as C

import pytest

import batch_auto_util as U

BLOCKS = (0, 1, 2, 3, 8191, 8192, 8193)
KINDS = [(f, u) for f in ("bc1", "bc2", "bc3") for u in (False, True)] + [("bc4", False), ("bc5", False)]


@pytest.fixture(scope="module")
def lib(pkg):
    return U.load(pkg)


def plan(lib, specs, chunk_capacity=4096):
    arr = U.make_items(specs)
    items = (U.PlanItem * max(1, len(specs)))()
    chunks = (U.PlanChunk * chunk_capacity)()
    n = C.c_size_t(123)
    rc = lib.dxtlt_debug_plan_batch_auto(arr, len(specs), items, chunks, chunk_capacity, C.byref(n))
    return rc, list(items[:len(specs)]), list(chunks[:min(n.value, chunk_capacity)]), n.value


def every_kind_and_count():
    specs, at = [], 0x10000000
    for fmt, use_all in KINDS:
        for blocks in BLOCKS:
            n = blocks * U.BLOCK[fmt]
            specs.append((fmt, at + 3, at + (1 << 20) + 1, n, use_all))     # any alignment: nothing is dereferenced
            at += 4 << 20
    return specs


def check_plan(specs, items, chunks):
    counters = []
    for k, ((fmt, _s, _d, n, use_all), it) in enumerate(zip(specs, items)):
        assert it.arena_offset % 16 == 0, k
        secs = list(it.sections[:it.section_count])
        assert [s.len for s in secs] == U.shown_lengths(fmt, n, use_all), (k, fmt, n, use_all)
        assert it.arena_bytes == sum(s.len for s in secs), k
        at = it.arena_offset
        for s in secs:                                                      # inside the slice, in slice order, disjoint
            assert s.arena_offset == at, (k, fmt)
            at += s.len
        assert at == it.arena_offset + it.arena_bytes
        counters += [s.counter for s in secs]
    assert len(counters) == len(set(counters)) and all(it.section_count <= 10 for it in items)
    assert sorted(counters) == list(range(len(counters)))                  # one dense buffer
    at = 0
    for c, ch in enumerate(chunks):                                         # chunks keep the item order and cover every item
        assert ch.first_item == at and ch.item_count >= 1, c
        mine = list(range(at, at + ch.item_count))
        at += ch.item_count
        assert all(items[i].chunk == c for i in mine)
        spans = sorted((items[i].arena_offset, items[i].arena_offset + items[i].arena_bytes) for i in mine)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), c       # slices disjoint within the chunk
        assert spans[-1][1] <= ch.arena_bytes
        wgs = sum(-(-s.len // U.WINDOW) for i in mine for s in items[i].sections[:items[i].section_count])
        assert ch.estimator_workgroups == wgs, c
        pairs = {(specs[i][0], bool(specs[i][4]) and specs[i][0] in ("bc1", "bc2", "bc3")) for i in mine if specs[i][3]}
        assert ch.candidate_launches <= len(pairs) and (ch.candidate_launches >= 1) == bool(pairs), c
    assert at == len(items)


def test_slices_sections_and_counters_of_every_format_and_count(lib):
    specs = every_kind_and_count()
    rc, items, chunks, n = plan(lib, specs)
    assert rc == 0 and n == 1 == len(chunks)
    check_plan(specs, items, chunks)
    assert chunks[0].candidate_launches == len(KINDS)
    assert items[0].section_count == 4 and items[len(BLOCKS)].section_count == 8        # bc1 fast, bc1 all modes: an empty item too


def test_chunks_under_a_small_cap(lib):
    specs = every_kind_and_count()
    whole = plan(lib, specs)[1]
    cap = 280_000                   # BC1 / BC2 with all modes: 32 bytes per block, 262 176 at 8193 blocks; BC3 with all modes: 36
    lib.dxtlt_debug_batch_auto_arena_cap(cap)
    try:
        rc, items, chunks, n = plan(lib, specs)
        small = plan(lib, specs, chunk_capacity=2)
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)
    assert rc == 0 and n == len(chunks) >= 8
    assert small[0] == 0 and small[3] == n and len(small[2]) == 2                        # counted, not written
    check_plan(specs, items, chunks)
    oversized = [i for i, it in enumerate(items) if it.arena_bytes > cap]
    assert oversized                                                                     # BC3 with all modes at 8192 and 8193 blocks: 294 912, 294 948
    for i in oversized:
        assert chunks[items[i].chunk].item_count == 1, i                                 # alone in its chunk
    for ch in chunks:
        assert ch.arena_bytes <= cap or ch.item_count == 1
    # a chunk is closed only when the next item would not fit
    for a, b in zip(chunks, chunks[1:]):
        nxt = items[b.first_item]
        assert a.arena_bytes + ((nxt.arena_bytes + 15) & ~15) > cap
    # sections and counters do not depend on the cap
    for a, b in zip(whole, items):
        assert [(s.len, s.counter) for s in a.sections[:a.section_count]] == [(s.len, s.counter) for s in b.sections[:b.section_count]]
    assert plan(lib, specs)[3] == 1                                                       # the default is back


def test_the_plan_validates_like_the_call(lib):
    ok = ("bc1", 0x1000, 0x9000, 64, False)
    assert plan(lib, [])[0] == 0
    assert lib.dxtlt_debug_plan_batch_auto(None, 3, None, None, 0, None) == 2
    assert lib.dxtlt_transform_batch_auto_device(None, 0, None) == 0
    assert lib.dxtlt_transform_batch_auto_device(None, 3, None) == 2
    for bad, status in ((("bc1", 0, 0x9000, 64, False), 2), (("bc1", 0x1000, 0, 64, False), 2), ((0, 0x1000, 0x9000, 64, False), 2),
                        ((6, 0x1000, 0x9000, 64, False), 2), ((7, 0x1000, 0x9000, 64, False), 2), (("bc1", 0x1000, 0x9000, 60, False), 1),
                        (("bc3", 0x1000, 0x9000, 24, True), 1), (("bc1", 0x1000, 0x1020, 64, False), 2)):     # the last: output over its input
        for specs in ([bad], [ok, bad], [bad, ok]):
            if bad[2] == 0x1020 and len(specs) == 2:
                specs = [("bc1", 0x20000, 0x30000, 64, False), bad]
            assert plan(lib, specs)[0] == status, bad
            arr = U.make_items(specs)
            assert lib.dxtlt_transform_batch_auto_device(arr, len(specs), None) == status, bad      # before any device work
            assert all(a.decorrelation_mode == 0xEE for a in arr)
    # two overlapping outputs; an output over another item's input; inputs may overlap one another
    assert plan(lib, [ok, ("bc2", 0x2000, 0x9030, 64, False)])[0] == 2
    assert plan(lib, [ok, ("bc2", 0x2000, 0x1038, 64, False)])[0] == 2
    assert plan(lib, [ok, ("bc2", 0x1000, 0xA000, 64, False)])[0] == 0
    assert plan(lib, [ok, ("bc2", 0, 0, 0, False)])[0] == 0                                          # an empty item needs no pointers
    # the winners' launch limit (2^24 - 1 tiles per format, len / block size / 256 + 2 per item) is part of the validation: three
    # BC1 items of 12 GiB are 18.9 million tiles; two are fine, and so are three of different formats
    big = [(f, (k + 1) << 40, ((k + 1) << 40) + (16 << 30), 12 << 30, False) for k, f in enumerate(("bc1", "bc1", "bc1"))]
    assert plan(lib, big)[0] == 2 and plan(lib, big[:2])[0] == 0
    arr = U.make_items(big)
    assert lib.dxtlt_transform_batch_auto_device(arr, 3, None) == 2 and all(a.decorrelation_mode == 0xEE for a in arr)
    assert plan(lib, [big[0], ("bc2",) + big[1][1:], ("bc3",) + big[2][1:]])[0] == 0
    assert plan(lib, [("bc1", 1 << 40, 1 << 41, 64 << 30, False)])[0] == 2                            # one item of 64 GiB


def test_the_two_estimator_kernels_keep_the_same_window_steps():
    """estimate_table_kernel carries a copy of estimate_kernel's steps on a window (csrc/estimate_kernels.hip says why): the two
    define the same integer, so from the window's first load to the last barrier they stay the same text, comments and the names
    of the two bounds aside."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dxt-lossless-transform_amd", "csrc",
                            "estimate_kernels.hip")).read()

    def steps(kernel):
        body = src[src.index(kernel):]
        body = body[body.index("const uintptr_t a = "):]
        body = body[:body.index("    if (tid == 0)\n        atomicAdd(", body.index("atomicAdd(&wg_matches"))]
        body = re.sub(r"//[^\n]*", "", body)
        body = re.sub(r"\blo_q\b", "lo", re.sub(r"\bhi_q\b", "hi", body))
        return [" ".join(l.split()) for l in body.splitlines() if l.strip()]

    a, b = steps(" estimate_kernel(const EstimateTable tab)"), steps("\nestimate_table_kernel(")
    assert len(a) > 40 and a == b


def test_a_batch_of_empty_items_reports_the_first_candidates_without_a_device(lib):
    specs = [(f, 0, 0, 0, u) for f, u in KINDS]
    arr = U.make_items(specs)
    assert lib.dxtlt_transform_batch_auto_device(arr, len(specs), None) == 0
    got = [(a.decorrelation_mode, a.split_alpha_endpoints, a.split_colour_endpoints) for a in arr[:len(specs)]]
    assert got == [(0, 0, 0), (2, 0, 0), (0, 0, 0), (2, 0, 0), (1, 1, 0), (2, 1, 0), (0, 0, 0), (0, 0, 0)]   # candidates_of(...)[0]
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    lib.dxtlt_debug_batch_auto_last(out)
    assert list(out) == [0, 0, 0, 0]
    assert lib.dxtlt_debug_batch_auto_last_totals(0, None, 0) == 0
