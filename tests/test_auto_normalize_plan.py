"""The auto transform with block normalisation (include/dxtlt_auto_normalize.h), everything that needs no device: the symbols and
their prototypes, the arena layout (dxtlt_debug_auto_normalization_sections == tests/auto_normalize_ref.py), the pick
(dxtlt_debug_auto_normalization_pick) with scripted sizes -- every candidate wins when it alone is smallest, a tie keeps the first in
candidate order, all-maximum sizes keep (None, Variant1, split) --, the answers to defective arguments, and the CPU statements on the
class-cycle data."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import auto_normalize_ref as A
from oracle import oracle_auto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = [(1, False), (1, True), (2, False), (2, True)]
SYMBOLS = ["dxtlt_transform_bc1_auto_with_normalization_device", "dxtlt_transform_bc2_auto_with_normalization_device",
           "dxtlt_transform_bc2_auto_with_normalization", "dxtlt_debug_auto_normalization_sections",
           "dxtlt_debug_auto_normalization_pick", "dxtlt_debug_auto_normalization_candidates_into_device",
           "dxtlt_debug_auto_normalization_last"]


@pytest.fixture(scope="module")
def lib(pkg):
    return A.load(pkg)


def test_symbols_exist_and_the_header_declares_them(lib):
    header = open(os.path.join(ROOT, "include", "dxtlt_auto_normalize.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name}: no prototype in include/dxtlt_auto_normalize.h"
    assert re.search(r"\bdxtlt_transform_bc1_auto_with_normalization\s*\(", open(os.path.join(ROOT, "include", "dxtlt_bc1_normalize.h")).read())
    for words in ("candidate index = norm * order_len", "6 x len", "12 x len", "3 x len", "wait 1", "wait 2"):
        assert words in header, words


@pytest.mark.parametrize("fmt,use_all", DEPTHS)
@pytest.mark.parametrize("blocks", [0, 1, 2, 513])
def test_sections_equal_the_python_layout(lib, fmt, use_all, blocks):
    off, length = (C.c_uint64 * 24)(*[77] * 24), (C.c_uint64 * 24)(*[77] * 24)
    count = lib.dxtlt_debug_auto_normalization_sections(fmt, use_all, blocks, off, length)
    want = A.sections(use_all, blocks)
    assert count == len(want) == (24 if use_all else 12)
    assert [(off[k], length[k]) for k in range(count)] == [(o, n) for _norm, _v, _sc, o, n in want]
    at = 0
    for k in range(count):                                   # end to end
        assert off[k] == at
        at += length[k]
    assert at == (96 if use_all else 48) * blocks == A.arena_bytes(use_all, blocks)
    assert list(off[count:]) == [77] * (24 - count)           # nothing behind the count is written
    for k, (norm, v, sc, _o, _n) in enumerate(want):
        assert A.section_index(use_all, norm, v, sc) == k


def test_sections_refuse_other_formats(lib):
    off, length = (C.c_uint64 * 24)(), (C.c_uint64 * 24)()
    for fmt in (0, 3, 4, 5, -1):
        assert lib.dxtlt_debug_auto_normalization_sections(fmt, False, 8, off, length) == -1


@pytest.mark.parametrize("fmt,use_all", DEPTHS)
def test_every_candidate_wins_when_it_alone_is_smallest(lib, fmt, use_all):
    cands = A.candidates(fmt, use_all)
    assert len(cands) == (24 if use_all else 12) and len(set(cands)) == len(cands)
    for c, (norm, v, sc) in enumerate(cands):
        sizes = [1000 + k for k in range(len(cands))]
        sizes[A.section_index(use_all, norm, v, sc)] = 10
        rc, choice, totals = A.pick(lib, fmt, use_all, sizes)
        assert rc == A.OK and choice == (norm, v, sc), (c, choice)
        assert totals == [sizes[A.section_index(use_all, *cand)] for cand in cands] and totals[c] == 10


@pytest.mark.parametrize("fmt,use_all", DEPTHS)
def test_a_tie_keeps_the_first_in_candidate_order(lib, fmt, use_all):
    cands = A.candidates(fmt, use_all)
    for first in range(len(cands)):
        for second in (first + 1, len(cands) - 1):
            if second <= first or second >= len(cands):
                continue
            sizes = [500] * len(cands)
            sizes[A.section_index(use_all, *cands[first])] = sizes[A.section_index(use_all, *cands[second])] = 7
            rc, choice, _totals = A.pick(lib, fmt, use_all, sizes)
            assert rc == A.OK and choice == cands[first], (first, second, choice)
    rc, choice, _totals = A.pick(lib, fmt, use_all, [5] * len(cands))     # all equal: candidate 0
    assert rc == A.OK and choice == cands[0]


@pytest.mark.parametrize("fmt,use_all", DEPTHS)
def test_all_maximum_sizes_keep_the_defaults(lib, fmt, use_all):
    n = 24 if use_all else 12
    rc, choice, totals = A.pick(lib, fmt, use_all, [A.U64_MAX] * n)
    assert rc == A.OK and choice == (A.NONE, 1, 1) and totals == [A.U64_MAX] * n
    sizes = [A.U64_MAX] * n                                             # and one below the maximum wins
    sizes[A.section_index(use_all, 2, 0, 0)] = A.U64_MAX - 1
    assert A.pick(lib, fmt, use_all, sizes)[1] == (2, 0, 0)


def test_pick_refuses_a_wrong_count_or_format(lib):
    for fmt, use_all, n in [(1, False, 24), (1, True, 12), (2, False, 11), (2, True, 25), (1, False, 0), (3, False, 12), (0, True, 24)]:
        rc, _choice, _totals = A.pick(lib, fmt, use_all, [1] * n)
        assert rc == A.E_ARGUMENT, (fmt, use_all, n)
    assert lib.dxtlt_debug_auto_normalization_pick(1, False, None, 12, None, 0, None, None, None) == A.E_ARGUMENT
    sizes = (C.c_uint64 * 12)(*range(12, 0, -1))                         # NULL outputs are allowed
    assert lib.dxtlt_debug_auto_normalization_pick(1, False, sizes, 12, None, 0, None, None, None) == A.OK


def test_validation_that_needs_no_device(lib):
    norm, mode, split = C.c_uint8(0xEE), C.c_uint8(0xEE), C.c_bool(False)
    outs = (C.byref(norm), C.byref(mode), C.byref(split))
    buf = (C.c_uint8 * 64)()
    at = C.addressof(buf)
    dev1, dev2 = lib.dxtlt_transform_bc1_auto_with_normalization_device, lib.dxtlt_transform_bc2_auto_with_normalization_device
    assert dev1(at, at, 12, False, None, *outs) == A.E_LENGTH and dev2(at, at, 24, True, None, *outs) == A.E_LENGTH
    assert dev1(None, at, 16, False, None, *outs) == A.E_ARGUMENT and dev1(at, None, 16, False, None, *outs) == A.E_ARGUMENT
    assert dev2(None, at, 16, False, None, *outs) == A.E_ARGUMENT and dev2(at, None, 32, True, None, *outs) == A.E_ARGUMENT
    est = lib.dxtlt_builtin_size_estimator()
    host2 = lib.dxtlt_transform_bc2_auto_with_normalization
    assert host2(at, at, 24, est, False, *outs, None) == A.E_LENGTH
    assert host2(at, at, 32, None, False, *outs, None) == A.E_ARGUMENT
    assert host2(None, at, 32, est, False, *outs, None) == A.E_ARGUMENT and host2(at, None, 32, est, True, *outs, None) == A.E_ARGUMENT
    hook = lib.dxtlt_debug_auto_normalization_candidates_into_device
    assert hook(3, False, at, 32, at, 1 << 20, None) == A.E_ARGUMENT and hook(1, False, at, 12, at, 1 << 20, None) == A.E_ARGUMENT
    assert hook(1, False, None, 0, None, 0, None) == A.OK
    assert (norm.value, mode.value) == (0xEE, 0xEE)                      # no refusal writes a result


# ---- the CPU statements on the class-cycle data --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 2])
def test_the_cycle_holds_every_class_in_every_slot(oracle, fmt):
    n = 4 * A.CYCLE + 1
    x = A.blocks(fmt, "cycle", n)
    bufs, any_normalized = A.normalized_buffers(fmt, x)
    assert any_normalized
    words = [np.ascontiguousarray(b).view("<u4").reshape(n, -1) for b in [x] + bufs]
    at = 0 if fmt == 1 else 2
    changed = [tuple(bool((w[b, at:at + 2] != words[0][b, at:at + 2]).any()) for w in words[1:]) for b in range(n)]
    cls = [A.class_of("cycle", fmt, b) for b in range(n)]
    by_class = {k: {changed[b] for b in range(n) if cls[b] == k} for k in range(A.CYCLE)}
    for k in (0, 11, 12):
        assert by_class[k] == {(False, False, False)}, k                  # unchanged under every mode
    for k in (2, 3, 6, 7, 10):
        assert by_class[k] == {(False, True, True)}, k                    # solid by an endpoint or by c0 == c1
    if fmt == 1:
        assert by_class[1] == by_class[9] == {(True, True, True)}         # transparent: rewritten in every buffer
    # both slots of a BC1 vector: class k occurs at an even and at an odd block, and the odd last block is a block of the cycle
    assert n % 2 == 1 and all({b % 2 for b in range(n) if cls[b] == k} == {0, 1} for k in range(A.CYCLE))
    none = A.blocks(fmt, "none", n)
    assert not A.normalized_buffers(fmt, none)[1]
    if fmt == 1:
        tr = A.blocks(1, "transparents", n)
        outs, any_tr = A.normalized_buffers(1, tr)
        assert any_tr and np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2]) and not np.array_equal(outs[0], tr)


@pytest.mark.parametrize("seed", [1, 2])
def test_bc2_solid_statement_agrees_with_the_oracles_normalisation(oracle, seed):
    """auto_normalize_ref.bc2_solid (decoded pixels) marks exactly the blocks the C oracle's BC2 ReplicateColor pass rewrites"""
    x = A.blocks(2, "cycle", 20 * A.CYCLE, seed=seed)
    v = np.ascontiguousarray(x).view("<u4").reshape(-1, 4)
    solid = A.bc2_solid(v[:, 2], v[:, 3])
    rep = np.ascontiguousarray(oracle.normalize_bc2_blocks(x, 2)).view("<u4").reshape(-1, 4)
    assert np.array_equal(solid, (rep[:, 2] != v[:, 2]) | (rep[:, 3] != v[:, 3]))    # the maker has no solid already in replicate form
    assert solid.any() and not solid.all()


@pytest.mark.parametrize("fmt,use_all", DEPTHS)
def test_every_mode_wins_on_some_data(oracle, fmt, use_all):
    """with estimator_ref.estimate: BC1's class cycle picks Color0Only, the solids with their random unused endpoints pick
    ReplicateColor (both formats), data without a normalisable block picks None through the plain statement"""
    for n in (4097, 20001):
        _x, (choice, out, totals, any_normalized) = A.case(fmt, "solids", n, use_all)
        assert any_normalized and len(totals) == (24 if use_all else 12) and out.size == n * A.BLOCK[fmt]
        assert choice[0] == A.REPLICATE_COLOR, (n, choice)
        assert choice == A.candidates(fmt, use_all)[totals.index(min(totals))]
        if fmt == 1:
            _x, (choice, _out, totals, any_normalized) = A.case(1, "cycle", n, use_all)
            assert any_normalized and choice[0] == A.COLOR0_ONLY, (n, choice)
            assert choice == A.candidates(1, use_all)[totals.index(min(totals))]
        _x, (choice, _out, totals, any_normalized) = A.case(fmt, "none", n, use_all)
        assert not any_normalized and choice[0] == A.NONE and len(totals) == (8 if use_all else 4)
        assert choice[1:] == tuple(oracle_auto.test_order(A.FMT[fmt], use_all)[totals.index(min(totals))][i] for i in (0, 2))


def test_bc1_none_winner_is_written_without_the_transparent_rewrite(oracle):
    """the statement's output for a None winner is the plain transform of the input, not of the buffer its candidates were estimated on"""
    x, (choice, out, _totals, any_normalized) = A.case(1, "transparents", 4097, False)
    assert any_normalized
    if choice[0] == A.NONE:
        assert np.array_equal(out, oracle.transform("bc1", x, choice[1], split_colour=bool(choice[2])))
