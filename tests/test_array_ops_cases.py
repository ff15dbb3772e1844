"""What the case lists of tests/array_ops_cases.py reach, proved without a device through dxtlt_debug_plan_array_op -- the plan
the launch functions of csrc/color565_ops.hip and csrc/bcn_decode.hip themselves take their route, lanes and grid from
(csrc/array_op_plan.h).  Every proof asserts exact counts, and first shows on a thinned list that it can fail."""
import ctypes as C

import numpy as np
import pytest

import array_ops_cases as K


@pytest.fixture(scope="module")
def lib(pkg):
    return K.declare(C.CDLL(pkg._lib.lib_path()))


# ---- the hook itself -------------------------------------------------------------------------------------------------------------------
def test_plan_hook_refuses_and_plans_nothing(lib):
    p = K.Plan()
    assert lib.dxtlt_debug_plan_array_op(3, 0, 0, 0, 8, C.byref(p)) == -1
    assert lib.dxtlt_debug_plan_array_op(K.OP_DECODE, 0, 0, 0, 8, C.byref(p)) == -1          # + format 1..3
    assert lib.dxtlt_debug_plan_array_op(K.OP_DIFFERENCE + 4, 0, 0, 0, 8, C.byref(p)) == -1
    assert lib.dxtlt_debug_plan_array_op(K.OP_YCOCG, 0, 0, 0, 8, None) == -1
    for op in (K.OP_YCOCG, K.OP_RECORRELATE_SPLIT, K.OP_SPLIT_ENDPOINTS, K.OP_DECODE + 1, K.OP_DIFFERENCE + 3):
        p = K.plan(lib, op, 0, 0, 0, 0)
        assert (p.vector, p.vector_lanes, p.single_lanes, p.workgroups, p.steps) == (0, 0, 0, 0, 0)


def test_plan_hook_on_hand_computed_cases(lib):
    def fields(p):
        return (p.vector, p.vector_lanes, p.single_lanes, p.workgroups, p.steps)

    assert fields(K.plan(lib, K.OP_YCOCG, 2051, 0x1000, 0x2010)) == (1, 256, 3, 2, 1)
    assert fields(K.plan(lib, K.OP_YCOCG, 2051, 0x1008, 0x2010)) == (0, 0, 2051, 9, 1)
    assert fields(K.plan(lib, K.OP_RECORRELATE_SPLIT, 1027, 0x1008, 0x3018, 0x2010)) == (1, 256, 3, 2, 1)
    assert fields(K.plan(lib, K.OP_RECORRELATE_SPLIT, 1027, 0x1008, 0x3018, 0x2018)) == (0, 0, 1027, 5, 1)
    assert fields(K.plan(lib, K.OP_SPLIT_ENDPOINTS, 2056, 0x1000, 0x2000)) == (1, 257, 0, 2, 1)
    assert fields(K.plan(lib, K.OP_SPLIT_ENDPOINTS, 2051, 0x1000, 0x2000)) == (0, 0, 2051, 9, 1)
    assert fields(K.plan(lib, K.OP_DECODE + 1, 259, 0x1008, 0x2000)) == (1, 259, 0, 2, 1)
    assert fields(K.plan(lib, K.OP_DECODE + 2, 259, 0x1008, 0x2000)) == (0, 0, 259, 2, 1)
    assert fields(K.plan(lib, K.OP_DIFFERENCE + 1, 513, 0x1008, 0x2008)) == (1, 513, 0, 2, 1)
    assert fields(K.plan(lib, K.OP_DIFFERENCE + 3, 513, 0x1008, 0x2000)) == (0, 0, 513, 2, 1)
    assert fields(K.plan(lib, K.OP_DIFFERENCE + 3, 4096 * 512, 0, 0)) == (1, 4096 * 512, 0, 4096, 1)
    assert fields(K.plan(lib, K.OP_DIFFERENCE + 3, 4096 * 512 + 1, 0, 0)) == (1, 4096 * 512 + 1, 0, 4096, 2)
    # past 2^32 lanes and at 64-bit addresses: the arithmetic is 64-bit
    assert fields(K.plan(lib, K.OP_YCOCG, (1 << 35) + 5, 1 << 40, 3 << 40)) == (1, 1 << 32, 5, (1 << 24) + 1, 1)
    assert fields(K.plan(lib, K.OP_YCOCG, 8, (1 << 40) + 8, 0)) == (0, 0, 8, 1, 1)


def test_host_slices_are_whole_blocks(lib):
    blocks, nbytes = K.slices(lib)
    assert blocks > 0 and blocks * 64 == 256 << 20                 # include/dxtlt_decode.h: 256 MiB of pixels
    assert nbytes == 256 << 20 and nbytes % 16 == 0


# ---- ycocg -----------------------------------------------------------------------------------------------------------------------------
def ycocg_offset_facts(lib, cases):
    """(pairs on the vector route, in-place cases on it, source residues met with destination 0, destination residues with source 0)"""
    vec = [c for c in cases if K.ycocg_plan(lib, c).vector]
    return ([c for c in vec if c[2] is not None], [c for c in vec if c[2] is None],
            sorted(s for _, s, d in cases if d == 0), sorted(d for _, s, d in cases if s == 0 and d is not None))


def test_ycocg_offset_list(lib):
    cases = K.ycocg_offset_cases()
    assert len(cases) == 272 == len(set(cases)) and {n for n, _, _ in cases} == {2051}
    # it can fail: without (0, 0) nothing out of place is on the vector route; even residues are half of them
    pairs, in_place, src, dst = ycocg_offset_facts(lib, [c for c in cases if c[1:] != (0, 0)])
    assert pairs == [] and len(in_place) == 1
    pairs, in_place, src, dst = ycocg_offset_facts(lib, [c for c in cases if c[1] % 2 == 0 and (c[2] or 0) % 2 == 0])
    assert src == dst == list(range(0, 16, 2))
    # the list
    pairs, in_place, src, dst = ycocg_offset_facts(lib, cases)
    assert pairs == [(2051, 0, 0)] and in_place == [(2051, 0, None)]
    assert src == dst == list(range(16))
    assert sorted(s for _, s, d in cases if d is None) == list(range(16))
    p = K.ycocg_plan(lib, (2051, 0, 0))
    assert (p.vector_lanes, p.single_lanes, p.workgroups) == (256, 3, 2)         # the singles start a workgroup of their own
    for c in cases:
        p = K.ycocg_plan(lib, c)
        if not p.vector:
            assert (p.vector_lanes, p.single_lanes, p.workgroups) == (0, 2051, 9)
    # every variant and both directions run all of it (tests/test_array_ops_sweep_gpu.py parametrises over exactly these)
    assert K.YCOCG_VARIANTS == (1, 2, 3)


def ycocg_count_facts(lib, cases):
    plans = [K.ycocg_plan(lib, c) for c in cases]
    vec = [p for p in plans if p.vector]
    full = [p for p in vec if p.vector_lanes % 256 == 0 and p.vector_lanes > 0 and p.single_lanes > 0]
    straddle = [p for p in vec if p.vector_lanes % 256 != 0 and p.single_lanes > 0
                and p.vector_lanes // 256 != (p.vector_lanes + p.single_lanes - 1) // 256]
    return len(vec), {p.single_lanes for p in vec}, len(full), len(straddle), {p.workgroups for p in plans}


def test_ycocg_count_list(lib):
    counts, cases = K.ycocg_counts(), K.ycocg_count_cases()
    assert len(counts) == 601 + 19 + 19 and len(cases) == 3 * 639 == len(set(cases))
    # it can fail: multiples of 8 have no singles; counts up to 600 stay in one workgroup
    assert ycocg_count_facts(lib, [c for c in cases if c[0] % 8 == 0])[1:4] == ({0}, 0, 0)
    assert ycocg_count_facts(lib, [c for c in cases if c[0] <= 600])[2:] == (0, 0, {0, 1})
    # the list: all three pointer pairs are 16-byte aligned, so every case with n > 0 is on the vector route
    n_vec, singles, full, straddle, wgs = ycocg_count_facts(lib, cases)
    assert n_vec == 3 * 638
    assert singles == set(range(8))
    # 2048 + 1..7 and 4096 + 1..7: singles behind a whole number of workgroups; 8 * 255 + 2..7, 8 * 511 + 2..7 and
    # 8 * 254 + 7, 8 * 510 + 7: singles that begin in one workgroup and end in the next
    assert full == 3 * 14 and straddle == 3 * 14
    assert wgs == {0, 1, 2, 3}


# ---- recorrelate split --------------------------------------------------------------------------------------------------------------------
def split_offset_facts(lib, cases):
    """(cases on the vector route, cases where the plan disagrees with the predicate, cases that violate only predicate 0 / 1 / 2)"""
    vec, wrong, alone = [], [], [0, 0, 0]
    for c in cases:
        _, s0, s1, d = c
        ok = (s0 % 8 == 0, s1 % 8 == 0, d % 16 == 0)
        p = K.split_plan(lib, c)
        if p.vector:
            vec.append(c)
        if bool(p.vector) != all(ok) or (p.vector_lanes, p.single_lanes) != ((256, 3) if all(ok) else (0, 1027)):
            wrong.append(c)
        if ok.count(False) == 1:
            alone[ok.index(False)] += 1
    return vec, wrong, alone


def test_split_offset_list(lib):
    cases = K.split_offset_cases()
    assert len(cases) == 16 * 16 * 8 == len(set(cases)) and {c[0] for c in cases} == {1027}
    # it can fail: one buffer cut in two (src1 = src0 + 2 * pairs, 6 mod 16 here: residues tied, as the older tests do) never has
    # both sources aligned, so it never reaches the vector route and never leaves the destination as the only obstacle
    tied = [c for c in cases if c[2] == (c[1] + 2 * 1027) % 16]
    vec, wrong, alone = split_offset_facts(lib, tied)
    assert len(tied) == 16 * 8 and (len(vec), wrong, alone[2]) == (0, [], 0)
    # the list
    vec, wrong, alone = split_offset_facts(lib, cases)
    assert wrong == []
    assert sorted(vec) == sorted((1027, s0, s1, d) for s0 in (0, 8) for s1 in (0, 8) for d in (0, 16))
    assert alone == [14 * 2 * 2, 2 * 14 * 2, 2 * 2 * 6]
    assert K.SPLIT_VARIANTS == (0, 1, 2, 3)


def test_split_count_list(lib):
    counts, cases = K.split_counts(), K.split_count_cases()
    assert len(counts) == 301 + 11 + 11 and len(cases) == 3 * 323 == len(set(cases))
    plans = [K.split_plan(lib, c) for c in cases]
    assert {p.single_lanes for p, c in zip(plans, cases) if p.vector and c[0] % 4 == 0} == {0}          # it can fail
    assert sum(p.vector for p in plans) == 3 * 322                                                     # all but pairs == 0
    assert {p.single_lanes for p in plans if p.vector} == {0, 1, 2, 3}
    assert all(p.vector_lanes == c[0] // 4 and p.single_lanes == c[0] % 4 for p, c in zip(plans, cases))
    assert {p.workgroups for p in plans} == {0, 1, 2, 3}                                               # 1024 + 1: 2; 2048 + 1: 3


# ---- split endpoints ------------------------------------------------------------------------------------------------------------------------
def endpoint_facts(lib, cases):
    vec, wrong, alone = [], [], [0, 0, 0]
    for c in cases:
        pairs, i, o = c
        ok = (i % 16 == 0, o % 16 == 0, pairs % 8 == 0)
        p = K.endpoint_plan(lib, c)
        if p.vector:
            vec.append(c)
        if bool(p.vector) != (all(ok) and pairs > 0) or p.vector_lanes != (pairs // 8 if p.vector else 0) \
                or p.single_lanes != (0 if p.vector else pairs):
            wrong.append(c)
        if ok.count(False) == 1:
            alone[ok.index(False)] += 1
    return vec, wrong, alone


def test_split_endpoint_lists(lib):
    offsets, counts = K.endpoint_offset_cases(), K.endpoint_count_cases()
    assert len(offsets) == 512 == len(set(offsets)) and len(counts) == 301 + 19
    # it can fail: the same shift on both pointers (the older tests) violates no pointer predicate alone; without 2051 the count
    # predicate is never the only one
    assert endpoint_facts(lib, [c for c in offsets if c[1] == c[2]])[2][:2] == [0, 0]
    assert endpoint_facts(lib, [c for c in offsets if c[0] == 2056])[2][2] == 0
    # the lists
    vec, wrong, alone = endpoint_facts(lib, offsets)
    assert vec == [(2056, 0, 0)] and wrong == [] and alone == [15, 15, 1]
    vec, wrong, alone = endpoint_facts(lib, counts)
    assert wrong == [] and vec == [c for c in counts if c[0] % 8 == 0 and c[0] > 0] and len(vec) == 37 + 3
    assert alone == [0, 0, len(counts) - 37 - 3 - 1]


# ---- decode -----------------------------------------------------------------------------------------------------------------------------------
def staged(lib, fmt, cases):
    return sorted(c[1:] for c in cases if K.decode_plan(lib, fmt, c).vector)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_decode_lists(lib, fmt):
    offsets, cases = K.decode_offset_cases(), K.decode_count_cases()
    assert len(offsets) == 17 * 17 == len(set(offsets)) and len(K.decode_counts()) == 131 + 7 + 7 and len(cases) == 4 * 145
    in_ok = (0, 8, 16) if fmt == "bc1" else (0, 16)
    # it can fail: residues 0..15 leave one aligned output and no second aligned input
    assert staged(lib, fmt, [c for c in offsets if c[1] < 16 and c[2] < 16]) == [(i, 0) for i in in_ok if i < 16]
    # the list
    assert staged(lib, fmt, offsets) == [(i, o) for i in in_ok for o in (0, 16)]
    for c in offsets:
        p = K.decode_plan(lib, fmt, c)
        assert (p.vector_lanes + p.single_lanes, p.workgroups, p.steps) == (259, 2, 1) and (p.single_lanes == 0) == bool(p.vector)
    assert 259 - 256 == 3                                                        # the second workgroup: three blocks of one wave
    routes = {ptr: {bool(K.decode_plan(lib, fmt, (n, *ptr)).vector) for n in K.decode_counts() if n} for ptr in K.DECODE_COUNT_POINTERS}
    assert routes == {(0, 0): {True}, (8, 0): {fmt == "bc1"}, (0, 8): {False}, (1, 1): {False}}
    assert {K.decode_plan(lib, fmt, c).workgroups for c in cases} == {0, 1, 2, 3}


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_block_pool_has_every_family(oracle, fmt):
    pool = K.block_pool(fmt)
    assert pool.shape == (K.POOL_BLOCKS, K.BLOCK[fmt]) and all(K.pool_window(n) + n <= K.POOL_BLOCKS for n in K.decode_counts() + [259])
    c0, c1 = K.colour_words(fmt, pool)
    assert min(int((c0 == c1).sum()), int((c0 < c1).sum()), int((c0 > c1).sum())) >= 100
    if fmt == "bc3":
        a0, a1 = pool[:, 0].astype(int), pool[:, 1].astype(int)
        assert min(int((a0 > a1).sum()), int((a0 < a1).sum())) >= 100 and int((a0 == a1).sum()) >= 1
        assert ((a0 == 0) & (a1 == 255)).any() and ((a0 == 255) & (a1 == 0)).any()
    assert len(np.unique(oracle.decode_blocks(fmt, pool.reshape(-1)).reshape(K.POOL_BLOCKS, 64), axis=0)) > 900


# ---- difference ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", K.FORMATS)
def test_difference_lengths(lib, fmt):
    lengths = K.difference_prefix_lengths()
    assert lengths == list(range(1, 1062)) and K.DIFF_BLOCKS == 2 * 512 + 37
    assert len({m % 512 for m in lengths if m < 512}) == 511                      # it can fail: one workgroup's worth misses residue 0
    assert sorted({m % 512 for m in lengths}) == list(range(512))
    for m in lengths:
        for a, b in K.DIFF_POINTERS:
            p = K.difference_plan(lib, fmt, m, a, b)
            assert (p.workgroups, p.steps) == ((m + 511) // 512, 1)
            assert bool(p.vector) == ((a, b) == (0, 0) or ((a, b) == (8, 8) and fmt == "bc1"))
    # the walk: two whole passes of the capped grid and a third step of the first workgroups
    assert K.WALK_BLOCKS == 2 * (1 << 21) + 512 + 37
    p = K.difference_plan(lib, fmt, K.WALK_BLOCKS - 549, 0, 0)
    assert (p.workgroups, p.steps) == (4096, 2)                                   # it can fail
    for a in (0, 1):
        p = K.difference_plan(lib, fmt, K.WALK_BLOCKS, a, 0)
        assert (p.workgroups, p.steps, bool(p.vector)) == (K.DIFF_GRID, 3, a == 0)


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_difference_pair_holds_the_three_kinds(oracle, fmt):
    """the flags the device test sums are the oracle's, and they are the kinds the arrays were built with"""
    for n, seed in ((K.DIFF_BLOCKS, 0xD1F0), (K.POOL_BLOCKS, 0xD1F1)):
        a, b = K.difference_pair(fmt, n, seed + K.KIND[fmt])
        kinds = K.block_kinds(n)
        pa, pb = (oracle.decode_blocks(fmt, x.reshape(-1)).reshape(n, 64) for x in (a, b))
        flags = (pa != pb).any(axis=1)
        bytes_differ = (a != b).any(axis=1)
        assert np.array_equal(flags, kinds == K.DIFFERENT) and np.array_equal(bytes_differ, kinds != K.EQUAL)
        assert [int((kinds == k).sum()) > n // 8 for k in (K.EQUAL, K.EQUIVALENT, K.DIFFERENT)] == [True] * 3
        assert flags[0] and flags[1:].any()             # some prefix begins and ends with a block whose pixels differ
        assert int(flags.sum()) == oracle.count_pixel_differences(fmt, a.reshape(-1), b.reshape(-1))
    a, b = K.solid_pair(fmt, K.POOL_BLOCKS)
    pa, pb = (oracle.decode_blocks(fmt, x.reshape(-1)).reshape(-1, 64) for x in (a, b))
    assert (pa != pb).any(axis=1).all() and (pa[:, 3::4] == 255).all()
