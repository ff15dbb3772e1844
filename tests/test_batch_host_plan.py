"""How dxtlt_transform_batch_host cuts a batch into chunks, checked without a GPU through dxtlt_debug_plan_batch_host
(include/dxtlt_gfx950.h): the hook runs the call's own planner (plan_host_batch, csrc/batch_host_plan.h), which is arithmetic over
the item lengths and the chunk cap.  Against a ten-line model of the rule and, independently of the model, the properties the call
relies on: which items go out alone, 256-byte slots that do not overlap, chunks that cover the rest in order, the chunk bound and
the arena bound.  tests/test_batch_host_small_gpu.py runs the pipeline over such a plan on the device."""
import ctypes as C
import itertools

import numpy as np
import pytest

from cabi import BATCH_HOST_ALONE as ALONE, plan_batch_host

KIB, MIB = 1 << 10, 1 << 20


@pytest.fixture(scope="module")
def lib(pkg):
    return C.CDLL(pkg._lib.lib_path())


def model(lens, cap):
    """the rule: items of two caps or more go out alone; the rest, in order, get 256-byte padded slots side by side, and a chunk is
    closed BEFORE the item that would push it past the cap, but only when it already holds bytes"""
    chunk_of, slot, chunks = [ALONE] * len(lens), [0] * len(lens), []
    for i, n in enumerate(lens):
        if n >= 2 * cap:
            continue
        padded = (n + 255) // 256 * 256
        if not chunks or (chunks[-1] > 0 and chunks[-1] + padded > cap):
            chunks.append(0)
        chunk_of[i], slot[i] = len(chunks) - 1, chunks[-1]
        chunks[-1] += padded
    return chunk_of, slot, chunks, max(chunks, default=0)


def check_properties(lens, cap, plan):
    chunk_of, slot, chunk_bytes, arena = plan
    packed = [i for i, n in enumerate(lens) if n < 2 * cap]
    for i, n in enumerate(lens):
        assert (chunk_of[i] == ALONE) == (n >= 2 * cap), (i, n, cap)
        assert slot[i] % 256 == 0
    # the chunks cover the items that do not go out alone, in order, without a gap
    assert [chunk_of[i] for i in packed] == sorted(chunk_of[i] for i in packed)
    assert sorted(set(chunk_of[i] for i in packed)) == list(range(len(chunk_bytes)))
    for c, nbytes in enumerate(chunk_bytes):
        members = [i for i in packed if chunk_of[i] == c]
        # slots: disjoint, inside the chunk, and the chunk ends with the last of them
        end = 0
        for i in sorted(members, key=lambda i: (slot[i], lens[i])):
            assert slot[i] >= end, (c, i)
            end = slot[i] + lens[i]
        assert end <= nbytes < end + 256 and nbytes % 256 == 0, (c, end, nbytes)
        # at most the cap, or exactly one non-empty item (of less than two caps) and empty ones
        assert nbytes <= cap or sum(1 for i in members if lens[i]) == 1, (c, nbytes, cap)
    assert arena == max(chunk_bytes, default=0) and arena < 3 * cap


def edge_lengths(cap):
    return [0, 1, 255, 256, 257, cap - 256, cap - 255, cap, cap + 1, 2 * cap - 1, 2 * cap, 2 * cap + 1]


@pytest.mark.parametrize("cap", [KIB, MIB])
def test_every_short_list_of_edge_lengths(lib, cap):
    """every list of up to 4 items drawn from the lengths at which the rule turns"""
    for n in range(5):
        for lens in itertools.product(edge_lengths(cap), repeat=n):
            plan = plan_batch_host(lib, lens, cap)
            assert plan == model(lens, cap), (lens, cap)
            check_properties(lens, cap, plan)


def test_random_lists_against_the_model(lib):
    rng = np.random.default_rng(0x4057B)
    for k in range(400):
        cap = int(rng.choice([KIB, 4 * KIB, 4 * KIB + 256, 64 * KIB, 100_000, MIB]))
        edges = edge_lengths(cap)
        lens = []
        for _ in range(int(rng.integers(1, 120))):
            kind = int(rng.integers(0, 6))
            lens.append(0 if kind == 0 else int(rng.choice(edges)) if kind == 1 else int(rng.integers(1, 600)) if kind == 2
                        else int(rng.integers(1, cap // 3)) if kind == 3 else int(rng.integers(1, 2 * cap)) if kind == 4
                        else int(rng.integers(2 * cap, 5 * cap)))
        plan = plan_batch_host(lib, lens, cap)
        assert plan == model(lens, cap), (k, cap, lens)
        check_properties(lens, cap, plan)


def test_the_chunk_is_closed_before_the_item_that_overfills_it(lib):
    """the cases the call's GPU tests reach only with hundreds of MiB: at the shipped cap of 64 MiB"""
    cap = 64 * MIB
    # a 30 MiB item, then 40 MiB items: one per chunk once the 30 MiB item sits in the first
    chunk_of, slot, chunks, arena = plan_batch_host(lib, [MIB, 30 * MIB, 40 * MIB, 40 * MIB, 136 * MIB, 8, 20 * MIB], cap)
    assert chunk_of == [0, 0, 1, 2, ALONE, 2, 2] and slot == [0, MIB, 0, 0, 0, 40 * MIB, 40 * MIB + 256]
    assert chunks == [31 * MIB, 40 * MIB, 60 * MIB + 256] and arena == 60 * MIB + 256
    # exactly the cap fits; one byte more does not; an item larger than the cap sits alone in its chunk, empties and all
    assert plan_batch_host(lib, [cap - 256, 256, 1], cap)[0] == [0, 0, 1]
    assert plan_batch_host(lib, [cap - 256, 257], cap)[0] == [0, 1]
    assert plan_batch_host(lib, [0, 0, 2 * cap - 1, 0, 5], cap) == ([0, 0, 0, 1, 1], [0, 0, 0, 0, 0], [2 * cap, 256], 2 * cap)
    # the threshold of the items that go out alone is two caps, on the unpadded length
    assert plan_batch_host(lib, [2 * cap - 1, 2 * cap, 2 * cap + 1], cap)[0] == [0, ALONE, ALONE]


def test_batches_without_work_for_the_pipeline(lib):
    """no item, only empty items, only items that go out alone: no chunk holds a byte and the arenas stay empty"""
    assert plan_batch_host(lib, [], MIB) == ([], [], [], 0)
    chunk_of, slot, chunks, arena = plan_batch_host(lib, [0] * 7, MIB)
    assert chunk_of == [0] * 7 and slot == [0] * 7 and sum(chunks) == 0 and arena == 0
    assert plan_batch_host(lib, [2 * MIB, 5 * MIB, 2 * MIB + 1], MIB) == ([ALONE] * 3, [0] * 3, [], 0)
    assert lib.dxtlt_debug_plan_batch_host(None, 3, C.c_uint64(MIB), None, None, None, 0, None) == -1
    assert lib.dxtlt_debug_plan_batch_host(None, 0, C.c_uint64(MIB), None, None, None, 0, None) == 0
