"""No device: why tests/test_auto_candidates_gpu.py compares bytes -- three wrong arenas whose estimates, all the auto calls ever
compare, are the right ones, each of which the byte comparison reports -- and what its case lists reach, counted here from the lists
themselves (tests/auto_candidates_ref.py) and from the call's own planner (dxtlt_debug_plan_batch_auto).  The last test thins the
lists and shows that the counts notice."""
import numpy as np
import pytest

import auto_candidates_ref as K
import estimator_ref as R


@pytest.fixture(scope="module")
def lib(pkg):
    return K.load(pkg)


# ---- what the totals cannot see ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,use_all", [(2, False), (3, True), (1, False)])
def test_the_totals_are_blind_to_what_the_byte_comparison_reports(oracle, fmt, use_all):
    n = 3 * K.WINDOW // 4 + 5                                   # colour sections of three windows and 20 bytes
    x = oracle.fill_splitmix64(n * K.BLOCK[fmt], 0x5EED + fmt)
    want = K.statement(oracle, fmt, use_all, x)
    secs = K.sections(fmt, use_all, n)
    estimates = [R.estimate(want[off:off + length]) for _n, off, length, _p in secs]
    assert all(length - 4 <= e <= length for e, (_n, _o, length, _p) in zip(estimates, secs))   # noise: hardly a gram of a window repeats

    def seen_and_hidden(mutated, size, word):
        assert [R.estimate(mutated[off:off + length]) for _n, off, length, _p in secs] == estimates      # the totals: blind
        arena = np.full(K.GUARD + size + K.GUARD, K.FILL, dtype=np.uint8)
        arena[K.GUARD:K.GUARD + mutated.size] = mutated
        report = K.differences(arena, [(K.GUARD, want, (fmt, use_all, n), "slice")])
        assert len(report) == 1 and word in report[0], report                                             # the bytes: seen
        return report[0]

    name, off, length, _per = secs[-2]                          # a colour pairs section
    assert length >= 2 * K.WINDOW
    # two 32 KiB windows of one section exchanged
    m = want.copy()
    m[off:off + K.WINDOW], m[off + K.WINDOW:off + 2 * K.WINDOW] = want[off + K.WINDOW:off + 2 * K.WINDOW], want[off:off + K.WINDOW]
    assert name in seen_and_hidden(m, want.size, "differ")
    # one byte changed: its four grams were unique and are unique
    m = want.copy()
    m[off + 4 * 1000 + 1] ^= 0x40
    line = seen_and_hidden(m, want.size, "differ")
    assert "1 of" in line and name in line and "(block 1000)" in line
    # bytes written behind the slice's end
    seen_and_hidden(np.concatenate([want, np.zeros(16, dtype=np.uint8)]), want.size + 16, "outside")
    # and the comparison itself: silent on the statement
    arena = np.full(K.GUARD + want.size + K.GUARD, K.FILL, dtype=np.uint8)
    arena[K.GUARD:K.GUARD + want.size] = want
    assert K.differences(arena, [(K.GUARD, want, (fmt, use_all, n), "slice")]) == []


def test_where_names_section_block_and_byte():
    n = 10
    assert K.where(3, False, n, 2 * 7 + 1) == "section 'alpha pairs' byte 15 (block 7)"
    assert K.where(3, False, n, 2 * n + n + 4) == "section 'alpha split' byte 14 (block 4)"
    assert K.where(3, False, n, 4 * n + 4 * 9) == "section 'colour pairs, variant 0' byte 36 (block 9)"
    assert K.where(3, False, n, 8 * n + 2 * n + 2 * 3 + 1) == "section 'colour split, variant 0' byte 27 (block 3)"
    assert K.where(5, False, n, 4 * n + 2) == "section 'green pairs' byte 2 (block 1)"
    assert [K.slice_bytes(f, u, 1) for f, u in K.GROUPS] == [16, 32, 16, 32, 20, 36, 4, 8]


# ---- what the case lists reach -------------------------------------------------------------------------------------------------------
def single_reach(small):
    """what the single kernel's list reaches, as the set of the claims of the GPU test's docstring that hold"""
    got = set()
    kernels = set()
    for fmt, use_all in K.SINGLE_GROUPS:
        jobs = K.single_jobs(fmt, small)
        for n, _off, _res in jobs:
            kernels.update(K.single_kernels(fmt, use_all, n))
        counts = [j[0] for j in jobs]
        w = K.workgroup_blocks(fmt)
        if {n % 8 for n in counts} == set(range(8)) and {2 * n % 16 for n in counts} == set(range(0, 16, 2)):
            got.add(("every N mod 8", fmt))
        if {n % 8 for n in counts if n < 64} == set(range(8)):
            got.add(("every N mod 8 inside one wave", fmt))
        if all(any(lo < n <= hi for n in counts) for lo, hi in ((0, w - 1), (w - 1, w), (w, 2 * w - 1), (2 * w, 4096))):
            got.add(("less than, exactly and more than a workgroup", fmt))
        if fmt == 1 and K.single_kernels(1, use_all, 1) == [("auto_candidates_bc1_last_block", use_all)] and 1 in counts:
            got.add(("the last-block kernel alone", use_all))
        if {(off, res % 128) for _n, off, res in jobs} == {(o, r) for o in K.INPUT_OFFSETS for r in K.ARENA_RESIDUES}:
            got.add(("every input offset with every arena residue", fmt))
    if len(kernels) == 6 + 2:
        got.add("all 6 + 2 single-buffer instantiations")
    return got


def batch_reach(lib, small):
    got = set()
    mixed = K.cases_mixed(small)
    if {c[:2] for c in mixed if c[2]} == set(K.GROUPS):
        got.add("all 8 batched instantiations")
    if {c[3] for c in mixed} == set(range(16)):
        got.add("every misalignment")
    if any(c[2] == 0 for c in mixed[1:-1]):
        got.add("an empty item in the middle")
    arms, halves = {}, {}
    for fmt, use_all, n, mis in mixed:
        if n == 0:
            continue
        lanes = (n + 1) // 2 if fmt in (1, 4) else n
        arms.setdefault((fmt, use_all), set()).update(K.load_arm(fmt, n, mis, v) for v in (0, lanes - 1))
        h = K.half_lane(fmt, n)
        if h is not None:
            wg, lane, lanes_of_wg = h
            halves.setdefault((fmt, use_all), set()).add("only lane" if (wg, lane) == (0, 0) else "last lane of a workgroup" if lane == 255
                                                         else "lane 0 of its own workgroup" if lane == 0 else "inside")
    if all(arms.get(g) == {"vector", "dword", "byte"} for g in K.GROUPS):
        got.add("all three load arms per launch")
    two_block = [g for g in K.GROUPS if g[0] in (1, 4)]
    for kind in ("only lane", "last lane of a workgroup", "lane 0 of its own workgroup"):
        if all(kind in halves.get(g, ()) for g in two_block):
            got.add("the half lane: " + kind)
    # the plan, from the call's own planner
    arr = K.fake_items(mixed)
    assert [arr[k].d_input % 16 for k in range(len(mixed))] == [c[3] for c in mixed]
    items, chunks = K.auto_plan(lib, arr, len(mixed))
    if len(chunks) == 1 and chunks[0].candidate_launches == 8:
        got.add("eight launches in one chunk")
    lib.dxtlt_debug_batch_auto_arena_cap(K.MIXED_CHUNK_CAP)
    try:
        cut_items, cut = K.auto_plan(lib, arr, len(mixed))
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)
    assert sorted({it.chunk for it in cut_items}) == list(range(len(cut)))
    assert all(cut_items[ch.first_item].arena_offset == 0 for ch in cut)                   # offsets restart per chunk
    if len(cut) >= 3 and all(ch.candidate_launches >= 1 for ch in cut) and all(ch.arena_bytes <= K.MIXED_CHUNK_CAP for ch in cut):
        got.add("three chunks or more, none empty")
    for it, c in zip(items, mixed):
        assert it.arena_bytes == K.slice_bytes(*c[:3]) and it.arena_offset % 16 == 0
        assert [(s.arena_offset - it.arena_offset, s.len) for s in it.sections[:it.section_count]] == [s[1:3] for s in K.sections(*c[:3])]
    if any(it.arena_bytes % 16 for it in items[:-1]):
        got.add("padding between two slices")
    return got


SINGLE_REACH = ({"all 6 + 2 single-buffer instantiations", ("the last-block kernel alone", False), ("the last-block kernel alone", True)}
                | {(what, fmt) for fmt in (1, 2, 3) for what in ("every N mod 8", "every N mod 8 inside one wave",
                                                                 "less than, exactly and more than a workgroup",
                                                                 "every input offset with every arena residue")})
BATCH_REACH = {"all 8 batched instantiations", "every misalignment", "an empty item in the middle", "all three load arms per launch",
               "the half lane: only lane", "the half lane: last lane of a workgroup", "the half lane: lane 0 of its own workgroup",
               "eight launches in one chunk", "three chunks or more, none empty", "padding between two slices"}


def test_the_case_lists_reach_what_they_claim(lib):
    assert single_reach(True) == SINGLE_REACH
    assert batch_reach(lib, True) == BATCH_REACH
    # the bisection
    deep = K.cases_deep()
    assert len(deep) == 300 and {c[:2] for c in deep} == {(1, False)} and K.bisection_steps(300) == 9
    assert K.bisection_steps(1) == 0 and K.bisection_steps(2) == 1 and [len(K.cases_count(k)) for k in (1, 2)] == [1, 2]
    assert {c[3] for c in deep} == set(range(16))
    assert {K.half_lane(c[0], c[2])[1] for c in deep if c[2] % 2} == {0, 255}
    _items, chunks = K.auto_plan(lib, K.fake_items(deep), 300)
    assert len(chunks) == 1 and chunks[0].candidate_launches == 1
    owners = K.cases_owners()
    assert [K.workgroups(c[0], c[2]) for c in owners] == [3, 2, 3] and len({c[:2] for c in owners}) == 1
    # every colour
    pairs = K.lane_pairs()
    assert pairs.shape == (8 * 65536, 2)
    for fmt in (1, 2):
        x = K.every_colour_blocks(fmt)
        dwords = K.colour_dwords(fmt, x)
        assert dwords.shape == ((x.size // 16), 2 if fmt == 1 else 1)
        for d in range(dwords.shape[1]):
            lo, hi = dwords[:, d] & 0xFFFF, dwords[:, d] >> 16
            for other in (0x0000, 0xFFFF):
                assert np.unique(lo[hi == other]).size == 65536 and np.unique(hi[lo == other]).size == 65536, (fmt, d, other)


def test_a_thinned_list_is_noticed(lib):
    """without the counts 1..66 (and the batch's items of one block) the counts above come out short"""
    single = single_reach(False)
    assert single < SINGLE_REACH
    assert SINGLE_REACH - single == ({("the last-block kernel alone", False), ("the last-block kernel alone", True)}
                                     | {("every N mod 8 inside one wave", fmt) for fmt in (1, 2, 3)})
    assert BATCH_REACH - batch_reach(lib, False) == {"the half lane: only lane"}


# ---- the hooks' argument checks ------------------------------------------------------------------------------------------------------
def test_the_hooks_check_their_arguments_before_any_device_work(lib):
    """made-up addresses, nothing is dereferenced"""
    single, batch = lib.dxtlt_debug_auto_candidates_into_device, lib.dxtlt_debug_batch_auto_candidates_device
    src, arena = 0x7000_0000_0000, 0x7100_0000_0000
    E = K.E_ARGUMENT
    assert single(0, False, src, 160, arena, 1 << 20, None) == E and single(4, False, src, 160, arena, 1 << 20, None) == E
    assert single(1, False, src, 164, arena, 1 << 20, None) == E and single(3, True, src, 168, arena, 1 << 20, None) == E
    assert single(2, False, src + 8, 160, arena, 1 << 20, None) == E and single(2, False, src, 160, arena + 4, 1 << 20, None) == E
    assert single(2, False, None, 160, arena, 1 << 20, None) == E and single(2, False, src, 160, None, 1 << 20, None) == E
    assert single(3, True, src, 160, arena, 359, None) == E and single(1, False, src, 168, arena, 21 * 16 - 1, None) == E
    assert single(1, True, None, 0, None, 0, None) == K.OK
    mixed = K.cases_mixed()
    arr = K.fake_items(mixed)
    _items, chunks = K.auto_plan(lib, arr, len(mixed))
    size = chunks[0].arena_bytes
    assert batch(arr, len(mixed), 1, arena, size, None) == E and b"chunk" in lib.dxtlt_last_error()
    assert batch(arr, len(mixed), 0, arena, size - 1, None) == E and b"arena" in lib.dxtlt_last_error()
    assert batch(arr, len(mixed), 0, None, size, None) == E and batch(arr, len(mixed), 0, arena + 8, size, None) == E
    assert batch(arr, 0, 0, arena, size, None) == E and batch(None, 3, 0, arena, size, None) == E
    arr[5].len += 1
    assert batch(arr, len(mixed), 0, arena, size, None) == K.E_LENGTH
    assert all(a.decorrelation_mode == 0xEE for a in arr[:len(mixed)])
