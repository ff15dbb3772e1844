"""What the tests of the auto transform with block normalisation share (tests/test_auto_normalize_plan.py,
tests/test_auto_normalize_gpu.py; include/dxtlt_auto_normalize.h, docs/ESTIMATOR.md "Auto transform with block normalisation"):
the CPU STATEMENTS of the call -- BC1: oracle_auto.transform_bc1_auto_with_normalization, BC2: composed here from
oracle_c.normalize_bc2_blocks, oracle_c.transform and the plain auto statement --, both with estimator_ref.estimate; the section
layout of the candidate kernel's arena and its statement; a data maker whose blocks cycle through every class of block in every
slot; and the ctypes view of the new symbols."""
from __future__ import annotations

import ctypes as C

import numpy as np

import estimator_ref as R
from oracle import oracle_auto, oracle_c

FMT = {1: "bc1", 2: "bc2"}
BLOCK = {1: 8, 2: 16}
OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
NONE, COLOR0_ONLY, REPLICATE_COLOR = 0, 1, 2
U64_MAX = 2**64 - 1
GUARD = 256
FILL = 0xEE


# ---- the layout: auto_normalize_sections (csrc/auto_launch.h) ---------------------------------------------------------------------
def variants(use_all):
    return 4 if use_all else 2


def sections(use_all, n):
    """[(norm, variant, split, offset, length)] of an arena of n blocks, in memory order: 12 or 24 sections of 4n bytes end to end"""
    out, at = [], 0
    for norm in range(3):
        for v in range(variants(use_all)):
            for sc in (0, 1):
                out.append((norm, v, sc, at, 4 * n))
                at += 4 * n
    return out


def arena_bytes(use_all, n):
    return (96 if use_all else 48) * n


def section_index(use_all, norm, v, sc):
    return norm * 2 * variants(use_all) + 2 * v + sc


def candidates(fmt, use_all):
    """[(norm, variant, split)] in candidate order: candidate index = norm * order_len + position in the format's test order"""
    return [(norm, v, sc) for norm in range(3) for v, _sa, sc in oracle_auto.test_order(FMT[fmt], use_all)]


# ---- the statements ---------------------------------------------------------------------------------------------------------------
def expand_565(v):
    r5, g6, b5 = (v >> 11) & 31, (v >> 5) & 63, v & 31
    return ((r5 << 3) | (r5 >> 2)) | (((g6 << 2) | (g6 >> 4)) << 8) | (((b5 << 3) | (b5 >> 2)) << 16)


def bc2_solid(colours, indices):
    """per block: whether the colour half (always four colours, alpha ignored) decodes to sixteen equal pixels of a colour that
    survives 8888 -> 565 -> 8888 -- from the decoded palette, not from the library's shortcut"""
    out = np.zeros(colours.size, dtype=bool)
    for b, (col, idx) in enumerate(zip(colours.tolist(), indices.tolist())):
        c0, c1 = col & 0xFFFF, col >> 16
        e0, e1 = expand_565(c0), expand_565(c1)
        ch0, ch1 = [(e0 >> s) & 255 for s in (0, 8, 16)], [(e1 >> s) & 255 for s in (0, 8, 16)]
        palette = [tuple(ch0), tuple(ch1), tuple((2 * a + b_) // 3 for a, b_ in zip(ch0, ch1)), tuple((a + 2 * b_) // 3 for a, b_ in zip(ch0, ch1))]
        pixels = {palette[(idx >> (2 * p)) & 3] for p in range(16)}
        if len(pixels) == 1:
            r, g, bl = next(iter(pixels))
            back = ((r & 0xF8) << 8) | ((g & 0xFC) << 3) | (bl >> 3)
            out[b] = expand_565(back) == (r | (g << 8) | (bl << 16))
    return out


def normalized_buffers(fmt, x):
    """(the three buffers the candidates are estimated on, any): BC1 normalize_blocks_all_modes (the None buffer with its transparent
    blocks rewritten), BC2 normalize_bc2_blocks per mode (None: the input)"""
    if fmt == 1:
        outs, any_normalized = oracle_c.normalize_bc1_blocks_all_modes(x)
        return [np.asarray(o) for o in outs], bool(any_normalized)
    v = np.ascontiguousarray(x).view("<u4").reshape(-1, 4)
    any_normalized = bool(bc2_solid(v[:, 2], v[:, 3]).any())
    return [np.asarray(x)] + [oracle_c.normalize_bc2_blocks(x, m) for m in (1, 2)], any_normalized


def colour_span(fmt, nbytes):
    return (0, nbytes // 2) if fmt == 1 else (nbytes // 2, 3 * nbytes // 4)


def arena_statement(fmt, use_all, x):
    """the expected arena for the AoS blocks x: every section the colour section of transform(normalized[norm], variant, split)"""
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    bufs, _any = normalized_buffers(fmt, x)
    a, b = colour_span(fmt, x.size)
    parts = [oracle_c.transform(FMT[fmt], bufs[norm], v, split_colour=bool(sc))[a:b] for norm, v, sc, _off, _len in sections(use_all, x.size // BLOCK[fmt])]
    out = np.concatenate(parts) if x.size else np.zeros(0, dtype=np.uint8)
    assert out.size == arena_bytes(use_all, x.size // BLOCK[fmt])
    return out


def call_statement(fmt, use_all, x, estimate=R.estimate):
    """((norm, variant, split), output bytes, totals in candidate order, any) of the whole call.  any == 0: the plain auto statement
    with its 4 / 8 totals."""
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    totals = []

    def recording(buf):
        totals.append(int(estimate(buf)))
        return totals[-1]

    if fmt == 1:
        _outs, any_normalized = oracle_c.normalize_bc1_blocks_all_modes(x)
        best, out, _calls = oracle_auto.transform_bc1_auto_with_normalization(x, recording, use_all)
        return tuple(int(b) for b in best), np.asarray(out), totals, bool(any_normalized)
    bufs, any_normalized = normalized_buffers(2, x)
    if not any_normalized:
        (v, _sa, sc), out, _calls = oracle_auto.transform_auto("bc2", x, recording, use_all)
        return (NONE, int(v), int(sc)), np.asarray(out), totals, False
    a, b = colour_span(2, x.size)
    best, best_size = (NONE, 1, 1), oracle_auto.SIZE_MAX
    for norm, v, sc in candidates(2, use_all):
        size = recording(oracle_c.transform("bc2", bufs[norm], v, split_colour=bool(sc))[a:b])
        if size < best_size:
            best_size, best = size, (norm, v, sc)
    out = oracle_c.transform("bc2", oracle_c.normalize_bc2_blocks(x, best[0]) if best[0] else x, best[1], split_colour=bool(best[2]))
    return best, np.asarray(out), totals, True


# ---- the data ---------------------------------------------------------------------------------------------------------------------
CYCLE = 13          # odd: both halves of a BC1 vector and the odd last block see every class
KINDS = ("none", "solids", "transparents", "cycle")


def class_of(kind, fmt, b):
    """the class (see blocks) of block b; the cycle starts so that blocks 0 and 1 of every kind but 'none' are blocks a mode changes"""
    if kind == "cycle":
        return (b + 1) % CYCLE
    if kind == "solids":
        k = (b + 2) % CYCLE
        return k if 2 <= k <= 10 and not (fmt == 1 and k == 9) else 0          # 9 is BC1's transparent twin
    if kind == "transparents":
        return 1 if b % CYCLE in (0, 5, 9) else 0
    return 11 if b % CYCLE == 11 else 0                                        # "none": plain blocks and the one that does not survive


def blocks(fmt, kind, n, seed=0):
    """n blocks of `kind`: 'cycle' runs through the 13 classes below in every slot, 'solids' keeps the solid ones, 'transparents'
    (BC1) the transparent ones, 'none' has no block that any mode changes.  Colours come from a small palette so that the colour
    sections have grams for the estimator to find; the endpoint no pixel of a solid block uses is random, as an encoder leaves it.
       0, 12  unchanged: c0 != c1, mixed indices            1  fully transparent (BC1: c0 <= c1, all indices 3; BC2: a solid by k = 3)
       2 - 5  all indices k = 0..3, four-colour order        6 - 9  all indices k = 0..3, three-colour order (9 = transparent for BC1)
       10     c0 == c1, mixed indices without 3              11     an interpolated colour that does not survive RGB565: unchanged"""
    assert kind in KINDS and (fmt == 1 or kind != "transparents")
    rng = np.random.default_rng([0xA0701, fmt, KINDS.index(kind), n, seed])
    palette = rng.integers(1, 0xFFFF, 48, dtype=np.uint32)
    colours, indices = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for b in range(n):
        k = class_of(kind, fmt, b)
        p, q = int(palette[(b // 5) % 48]), int(palette[(b // 5 + 7) % 48])
        hi, lo = max(p, q), min(p, q)
        if hi == lo:
            hi, lo = lo + 1, lo
        mixed = (int(rng.integers(0, 1 << 32)) & ~0xF) | 0x4            # pixel 0 has index 0, pixel 1 index 1
        if k in (0, 12):
            c0, c1, idx = (hi, lo, mixed) if k == 0 else (lo, hi, mixed)
        elif k == 1:
            c0, c1, idx = lo, hi, 0xFFFFFFFF
        elif 2 <= k <= 5:
            c0, c1, idx = hi, lo, (k - 2) * 0x55555555
            if k == 2:
                c1 = int(rng.integers(0, hi))                        # a flat area: the pixels' colour from the palette, the endpoint
            elif k == 3:                                             # no pixel uses whatever the encoder left there
                c0 = int(rng.integers(lo + 1, 0x10000))
        elif 6 <= k <= 9:
            c0, c1, idx = lo, hi, (k - 6) * 0x55555555
            if k == 6:
                c1 = int(rng.integers(lo, 0x10000))
            elif k == 7:
                c0 = int(rng.integers(0, hi + 1))
        elif k == 10:
            c0, c1, idx = hi, hi, (mixed & 0x55555545) | 0x20         # index values 0 and 1, pixel 2 has index 2: never 3
        else:
            c0, c1, idx = 0xFFFF, 0x0000, 0xAAAAAAAA                   # (2 * 255 + 0) / 3 = 170: 565 gives back 173
        colours[b], indices[b] = c0 | (c1 << 16), idx
    if fmt == 1:
        out = np.stack([colours, indices], axis=1).astype("<u4")
    else:
        alpha = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint32)
        out = np.concatenate([alpha, colours[:, None], indices[:, None]], axis=1).astype("<u4")
    out = np.ascontiguousarray(out).view(np.uint8).reshape(-1)
    assert out.size == n * BLOCK[fmt]
    return out


_CASES = {}


def case(fmt, kind, n, use_all):
    """(blocks, call statement), read-only, computed once per session"""
    key = (fmt, kind, n, use_all)
    if key not in _CASES:
        x = blocks(fmt, kind, n)
        x.setflags(write=False)
        _CASES[key] = (x, call_statement(fmt, use_all, x))
    return _CASES[key]


_ARENAS = {}


def arena_case(fmt, use_all, n):
    key = (fmt, use_all, n)
    if key not in _ARENAS:
        x = blocks(fmt, "cycle", n, seed=1)
        want = arena_statement(fmt, use_all, x)
        x.setflags(write=False)
        want.setflags(write=False)
        _ARENAS[key] = (x, want)
    return _ARENAS[key]


# ---- the library ------------------------------------------------------------------------------------------------------------------
def load(pkg):
    """the library with every symbol these tests call declared: a missing symbol raises AttributeError here, a failure"""
    l = C.CDLL(pkg._lib.lib_path())
    vp, sz, i32, u64, b = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64, C.c_bool
    u8p, bp, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_bool), C.POINTER(u64)
    for n in (1, 2):
        f = getattr(l, f"dxtlt_transform_bc{n}_auto_with_normalization_device")
        f.argtypes, f.restype = [vp, vp, sz, b, vp, u8p, u8p, bp], i32
        f = getattr(l, f"dxtlt_transform_bc{n}_auto_with_normalization")
        f.argtypes, f.restype = [vp, vp, sz, vp, b, u8p, u8p, bp, C.POINTER(C.c_uint32)], i32
        f = getattr(l, f"dxtlt_transform_bc{n}_auto_device")
        f.argtypes, f.restype = [vp, vp, sz, b, vp, u8p, bp], i32
    l.dxtlt_debug_auto_normalization_sections.argtypes = [i32, b, u64, u64p, u64p]
    l.dxtlt_debug_auto_normalization_sections.restype = i32
    l.dxtlt_debug_auto_normalization_pick.argtypes = [i32, b, u64p, i32, u64p, i32, u8p, u8p, bp]
    l.dxtlt_debug_auto_normalization_pick.restype = i32
    l.dxtlt_debug_auto_normalization_candidates_into_device.argtypes = [i32, b, vp, sz, vp, u64, vp]
    l.dxtlt_debug_auto_normalization_candidates_into_device.restype = i32
    l.dxtlt_debug_auto_normalization_last.argtypes, l.dxtlt_debug_auto_normalization_last.restype = [u64p], None
    l.dxtlt_debug_auto_last_totals.argtypes, l.dxtlt_debug_auto_last_totals.restype = [u64p, i32], i32
    l.dxtlt_debug_auto_last_estimation.argtypes, l.dxtlt_debug_auto_last_estimation.restype = [u64p, u64p], None
    l.dxtlt_debug_auto_use_arena.argtypes, l.dxtlt_debug_auto_use_arena.restype = [i32], None
    l.dxtlt_builtin_size_estimator.argtypes, l.dxtlt_builtin_size_estimator.restype = [], vp
    l.dxtlt_last_error.argtypes, l.dxtlt_last_error.restype = [], C.c_char_p
    return l


def last(lib):
    out = (C.c_uint64 * 4)()
    lib.dxtlt_debug_auto_normalization_last(out)
    return list(out)


def last_totals(lib):
    out = (C.c_uint64 * 32)()
    n = lib.dxtlt_debug_auto_last_totals(out, 32)
    return list(out[:n])


def last_estimation(lib):
    a, b = C.c_uint64(99), C.c_uint64(99)
    lib.dxtlt_debug_auto_last_estimation(C.byref(a), C.byref(b))
    return a.value, b.value


def pick(lib, fmt, use_all, sizes):
    """(status, (norm, mode, split), totals) of dxtlt_debug_auto_normalization_pick"""
    n = len(sizes)
    arr, totals = (C.c_uint64 * max(1, n))(*sizes), (C.c_uint64 * 24)()
    norm, mode, split = C.c_uint8(0xEE), C.c_uint8(0xEE), C.c_bool(False)
    rc = lib.dxtlt_debug_auto_normalization_pick(fmt, use_all, arr, n, totals, 24, C.byref(norm), C.byref(mode), C.byref(split))
    return rc, (norm.value, mode.value, int(split.value)), list(totals[:n]) if rc == OK else None
