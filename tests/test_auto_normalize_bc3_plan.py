"""BC3's auto transform with block normalisation (include/dxtlt_auto_normalize.h), everything that needs no device: the symbols and
their prototypes, the arena layout (dxtlt_debug_bc3_auto_normalization_sections == tests/auto_normalize_bc3_ref.py), the pick
(dxtlt_debug_bc3_auto_normalization_pick) against a Python fold -- random sizes, every one of the 96 / 192 candidates scripted as the
unique minimum, all sizes equal, one wrapping sum --, SEPARABILITY (the literal walk of 96 / 192 full CPU transforms gives the totals
the sums over 20 / 32 section estimates give), the data maker's class pairs, the modes the CPU statement picks, and the answers to
defective arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import auto_normalize_bc3_ref as B
import auto_normalize_ref as A
import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dxtlt_transform_bc3_auto_with_normalization_device", "dxtlt_transform_bc3_auto_with_normalization",
           "dxtlt_debug_bc3_auto_normalization_sections", "dxtlt_debug_bc3_auto_normalization_pick",
           "dxtlt_debug_bc3_auto_normalization_candidates_into_device"]
# data kind -> the (alpha mode, colour mode) the CPU statement picks on it; between them every mode of both kinds
WINNERS = {"none": (0, 0), "unchanged": (0, 0), "uniform": (1, 0), "opaque": (2, 0), "zero": (3, 0), "cycle": (3, 2), "color0": (0, 1)}


@pytest.fixture(scope="module")
def lib(pkg):
    return B.load(pkg)


def test_symbols_exist_and_the_header_declares_them(lib):
    header = open(os.path.join(ROOT, "include", "dxtlt_auto_normalize.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name}: no prototype in include/dxtlt_auto_normalize.h"
    for words in ("(alpha_mode * 3 + colour_mode) * order_len + position", "2 * alpha_mode + split_alpha",
                  "8 + colour_mode * (2 * variants) + 2 * variant + split_colour", "4 x len or 7 x len", "20 / 32"):
        assert words in header, words
    assert "Out of scope:\n * transform_bc3_auto_with_normalization" not in open(os.path.join(ROOT, "include", "dxtlt_bc23_normalize.h")).read()


def test_the_rust_sys_crate_declares_both_calls_with_the_headers_types():
    """the `-sys` crate's block for include/dxtlt_auto_normalize.h (test_cabi_load.py checks the crate's first block only): the same
    parameters in order, with the header's names and the types the fixed C -> Rust mapping gives"""
    from test_cabi_load import _split_args, _strip_c_comments, c_type_to_rust, rust_type

    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust", "dxt-lossless-transform-gfx950-sys", "src", "lib.rs")).read())
    header = _strip_c_comments(open(os.path.join(ROOT, "include", "dxtlt_auto_normalize.h")).read())
    for name in SYMBOLS[:2]:
        r = re.search(r"pub fn " + name + r"\(([^)]*)\)\s*->\s*([^;]+);", src)
        c = re.search(r"([\w ]+?[\s\*]+)\b" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert r and c, name
        assert rust_type(r.group(2)) == c_type_to_rust(c.group(1), named=False) == "i32"
        c_args, rust_args = _split_args(c.group(2)), _split_args(r.group(1))
        assert len(c_args) == len(rust_args) == (10 if name.endswith("_device") else 11), (name, c_args, rust_args)
        for ca, ra in zip(c_args, rust_args):
            rname, rty = [v.strip() for v in ra.split(":", 1)]
            assert rust_type(rty) == c_type_to_rust(ca) and rname == ca.replace("*", " ").split()[-1], (name, ca, ra)


@pytest.mark.parametrize("use_all", [False, True])
@pytest.mark.parametrize("blocks", [0, 1, 2, 513])
def test_sections_equal_the_python_layout(lib, use_all, blocks):
    off, length = (C.c_uint64 * 32)(*[77] * 32), (C.c_uint64 * 32)(*[77] * 32)
    count = lib.dxtlt_debug_bc3_auto_normalization_sections(use_all, blocks, off, length)
    want = B.sections(use_all, blocks)
    assert count == len(want) == B.section_count(use_all) == (32 if use_all else 20)
    assert [(off[k], length[k]) for k in range(count)] == [(o, n) for _key, o, n in want]
    at = 0
    for k in range(count):                                   # end to end
        assert off[k] == at
        at += length[k]
    assert at == (112 if use_all else 64) * blocks == B.arena_bytes(use_all, blocks)
    assert list(off[count:]) == [77] * (32 - count)           # nothing behind the count is written
    for k, (key, _o, _n) in enumerate(want):
        assert (B.alpha_index(*key[1:]) if key[0] == "a" else B.colour_index(use_all, *key[1:])) == k
    # the colour part starts at 16N and is BC2's arena
    bc2 = A.sections(use_all, blocks)
    assert [(o - 16 * blocks, n) for _key, o, n in want[8:]] == [(o, n) for _norm, _v, _sc, o, n in bc2]
    assert [key[1:] for key, _o, _n in want[8:]] == [(norm, v, sc) for norm, v, sc, _o, _n in bc2]


def test_the_older_hooks_still_refuse_format_3(lib):
    off, length = (C.c_uint64 * 24)(), (C.c_uint64 * 24)()
    assert lib.dxtlt_debug_auto_normalization_sections(3, False, 8, off, length) == -1
    assert A.pick(lib, 3, False, [1] * 12)[0] == A.E_ARGUMENT


def test_candidate_numbering():
    for use_all in (False, True):
        cands = B.candidates(use_all)
        order = len(cands) // 12
        assert len(cands) == (192 if use_all else 96) and len(set(cands)) == len(cands) and order == (16 if use_all else 8)
        for k, (am, cm, _v, _sa, _sc) in enumerate(cands):
            assert k // order == am * 3 + cm
        assert len({(B.alpha_index(am, sa), B.colour_index(use_all, cm, v, sc)) for am, cm, v, sa, sc in cands}) == len(cands)


@pytest.mark.parametrize("use_all", [False, True])
def test_pick_equals_the_fold_on_random_sizes(lib, use_all):
    rng = np.random.default_rng([0xB3, int(use_all)])
    n = B.section_count(use_all)
    for trial in range(200):
        hi = (4, 50, 1 << 20, 1 << 62)[trial % 4]              # small ranges make ties
        sizes = [int(v) for v in rng.integers(0, hi, n)]
        rc, choice, totals = B.pick(lib, use_all, sizes)
        want_choice, want_totals = B.fold(use_all, sizes)
        assert rc == B.OK and choice == want_choice and totals == want_totals, (trial, sizes)


@pytest.mark.parametrize("use_all", [False, True])
def test_every_candidate_wins_when_it_alone_is_smallest(lib, use_all):
    cands = B.candidates(use_all)
    n = B.section_count(use_all)
    for c, (am, cm, v, sa, sc) in enumerate(cands):
        sizes = [1000 + 3 * k for k in range(n)]
        sizes[B.alpha_index(am, sa)] = 10
        sizes[B.colour_index(use_all, cm, v, sc)] = 7
        rc, choice, totals = B.pick(lib, use_all, sizes)
        assert rc == B.OK and choice == (am, cm, v, sa, sc), (c, choice)
        assert totals[c] == 17 and sorted(totals)[1] > 17 and totals == B.fold(use_all, sizes)[1]


@pytest.mark.parametrize("use_all", [False, True])
def test_equal_sizes_keep_candidate_0_and_maximum_sums_keep_the_defaults(lib, use_all):
    n = B.section_count(use_all)
    cands = B.candidates(use_all)
    rc, choice, totals = B.pick(lib, use_all, [5] * n)
    assert rc == B.OK and choice == cands[0] and totals == [10] * len(cands)
    sizes = [0] * 8 + [B.U64_MAX] * (n - 8)                    # every sum is the maximum: nothing is below the initial best
    rc, choice, totals = B.pick(lib, use_all, sizes)
    assert rc == B.OK and choice == (0, 0, 1, 1, 1) and totals == [B.U64_MAX] * len(cands)
    sizes[B.colour_index(use_all, 2, 0, 1)] = B.U64_MAX - 1      # and one below it wins, with the first alpha section of its kind
    first = next(c for c in cands if c[1:3] == (2, 0) and c[4] == 1)
    assert B.pick(lib, use_all, sizes)[1] == first


@pytest.mark.parametrize("use_all", [False, True])
def test_the_sum_wraps_as_the_plain_call_does(lib, use_all):
    n = B.section_count(use_all)
    sizes = [1 << 40] * n
    am, cm, v, sa, sc = B.candidates(use_all)[-3]
    sizes[B.alpha_index(am, sa)] = B.U64_MAX - 2
    sizes[B.colour_index(use_all, cm, v, sc)] = 8               # (2^64 - 3 + 8) mod 2^64 = 5
    rc, choice, totals = B.pick(lib, use_all, sizes)
    assert rc == B.OK and totals == B.fold(use_all, sizes)[1] and totals[-3] == 5
    assert choice == (am, cm, v, sa, sc)


def test_pick_refuses_a_wrong_count(lib):
    for use_all, n in [(False, 32), (True, 20), (False, 12), (True, 24), (False, 0), (False, 19), (True, 33)]:
        assert B.pick(lib, use_all, [1] * n)[0] == B.E_ARGUMENT, (use_all, n)
    assert lib.dxtlt_debug_bc3_auto_normalization_pick(False, None, 20, None, 0, None, None, None, None, None) == B.E_ARGUMENT
    sizes = (C.c_uint64 * 20)(*range(20, 0, -1))                 # NULL outputs are allowed
    assert lib.dxtlt_debug_bc3_auto_normalization_pick(False, sizes, 20, None, 0, None, None, None, None, None) == B.OK


def test_validation_that_needs_no_device(lib):
    outs = B.Outs()
    buf = (C.c_uint8 * 64)()
    at = C.addressof(buf)
    dev = lib.dxtlt_transform_bc3_auto_with_normalization_device
    assert dev(at, at, 24, False, None, *outs.refs()) == B.E_LENGTH and dev(at, at, 8, True, None, *outs.refs()) == B.E_LENGTH
    assert dev(None, at, 16, False, None, *outs.refs()) == B.E_ARGUMENT and dev(at, None, 32, True, None, *outs.refs()) == B.E_ARGUMENT
    est = lib.dxtlt_builtin_size_estimator()
    host = lib.dxtlt_transform_bc3_auto_with_normalization
    assert host(at, at, 24, est, False, *outs.refs(), None) == B.E_LENGTH
    assert host(at, at, 32, None, False, *outs.refs(), None) == B.E_ARGUMENT
    assert host(None, at, 32, est, False, *outs.refs(), None) == B.E_ARGUMENT and host(at, None, 32, est, True, *outs.refs(), None) == B.E_ARGUMENT
    hook = lib.dxtlt_debug_bc3_auto_normalization_candidates_into_device
    assert hook(False, at, 24, at, 1 << 20, None) == B.E_ARGUMENT
    assert hook(False, None, 0, None, 0, None) == B.OK
    assert outs.untouched()                                       # no refusal writes a result


# ---- the CPU statement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_all", [False, True])
def test_the_totals_are_separable(oracle, use_all):
    """the literal walk -- one full CPU normalise + transform per candidate, 96 and 192 of them -- gives the totals that the sums over
    the 20 / 32 section estimates give: what lets the device flow produce and estimate the distinct sections only"""
    x, (choice, _out, totals, any_normalized) = B.case("cycle", 4097, use_all)
    assert any_normalized and len(totals) == (192 if use_all else 96)
    assert B.literal_totals(use_all, x) == totals
    assert choice == B.candidates(use_all)[totals.index(min(totals))]


def test_the_data_holds_every_pair_of_classes(oracle):
    n = B.ALPHA_CYCLE * A.CYCLE
    x = B.blocks("cycle", n)
    pairs = {(B.alpha_class_of("cycle", b), A.class_of("cycle", 2, b)) for b in range(n)}
    assert len(pairs) == n and B.ALPHA_CYCLE % 2 == 1 and np.gcd(B.ALPHA_CYCLE, A.CYCLE) == 1
    v = np.ascontiguousarray(x).view("<u4").reshape(-1, 4)
    uniform = B.alpha_uniform(v[:, 0], v[:, 1])
    by_class = {k: {bool(uniform[b]) for b in range(n) if B.alpha_class_of("cycle", b) == k} for k in range(B.ALPHA_CYCLE)}
    for k in range(B.ALPHA_CYCLE):
        assert by_class[k] == {k not in (0, 18, 24)}, k             # the statement's walk agrees with what each class is made to be
    # the classifier the library runs agrees with the decoded values: the C oracle's mode 1 changes or keeps exactly the uniform halves
    one = np.ascontiguousarray(oracle.normalize_bc3_blocks(x, 1, 0)).view("<u4").reshape(-1, 4)
    normal_form = (v[:, 0] < 256) & (v[:, 1] == 0)                 # (alpha, 0) with indices 0: uniform, and already what mode 1 writes
    assert np.array_equal(uniform, (one[:, 0] != v[:, 0]) | (one[:, 1] != v[:, 1]) | normal_form)
    # 255 by index 7 and 0 by index 6 occur, and the unchanged kinds
    pairs_of = lambda k: {int(v[b, 0]) & 0xFFFF for b in range(n) if B.alpha_class_of("cycle", b) == k}
    assert pairs_of(21) == {0xFFFF} and pairs_of(22) == {0} and all(p >> 8 == 0 for p in pairs_of(23))
    assert not B.any_normalizable(B.blocks("none", n)) and B.any_normalizable(B.blocks("unchanged", n))


@pytest.mark.parametrize("use_all", [False, True])
def test_every_mode_wins_on_some_data(oracle, use_all):
    """with estimator_ref.estimate, at both sizes the device test runs: every alpha mode and every colour mode is the winner's on
    some data kind"""
    for n in (4097, 20001):
        won_alpha, won_colour = set(), set()
        for kind, (alpha_mode, colour_mode) in WINNERS.items():
            _x, (choice, out, totals, any_normalized) = B.case(kind, n, use_all)
            assert choice[:2] == (alpha_mode, colour_mode), (kind, n, choice)
            assert out.size == 16 * n and any_normalized == (kind != "none")
            if any_normalized:
                assert len(totals) == (192 if use_all else 96) and choice == B.candidates(use_all)[totals.index(min(totals))]
            else:
                assert len(totals) == (16 if use_all else 8)
            won_alpha.add(choice[0])
            won_colour.add(choice[1])
        assert won_alpha == {0, 1, 2, 3} and won_colour == {0, 1, 2}


def test_a_scripted_estimator_sees_the_statement_through(oracle):
    """call_statement with another estimator (the callback route's statement): the fold over its answers"""
    x = B.blocks("cycle", 27)
    est = lambda buf: cabi.section_key(buf)[1] & 0xFFFF
    choice, out, totals, any_normalized = B.call_statement(False, x, estimate=est)
    assert any_normalized and totals == B.literal_totals(False, x, estimate=est)
    am, cm, v, sa, sc = choice
    assert np.array_equal(out, oracle.transform("bc3", oracle.normalize_bc3_blocks(x, am, cm), v, split_colour=bool(sc), split_alpha=bool(sa)))
