"""What the tests of BC3's auto transform with block normalisation share (tests/test_auto_normalize_bc3_plan.py,
tests/test_auto_normalize_bc3_gpu.py; include/dxtlt_auto_normalize.h, docs/ESTIMATOR.md "Auto transform with block normalisation"):
the CPU STATEMENT of the call, built from oracle_c.normalize_bc3_blocks, oracle_c.transform, oracle_auto.test_order("bc3", ...),
oracle_auto.transform_auto and estimator_ref.estimate -- as the literal walk (one full transform per candidate) and as the sums over
the distinct sections the device flow estimates --; the section layout of the candidate kernel's arena and its statement; a data
maker whose alpha halves cycle through every class of alpha half while the colour halves cycle through auto_normalize_ref's
classes; and the ctypes view of the new symbols."""
from __future__ import annotations

import ctypes as C

import numpy as np

import auto_normalize_ref as A
import estimator_ref as R
from oracle import oracle_auto, oracle_c

OK, E_LENGTH, E_ARGUMENT, E_ESTIMATOR = 0, 1, 2, 5
U64 = 1 << 64
U64_MAX = U64 - 1
GUARD = 256
FILL = 0xEE
ALPHA_SECTIONS = 8
MAX_SECTIONS, MAX_CANDIDATES = 32, 192


# ---- the layout: auto_normalize_bc3_sections (csrc/auto_launch.h) -----------------------------------------------------------------
def variants(use_all):
    return 4 if use_all else 2


def section_count(use_all):
    return ALPHA_SECTIONS + 6 * variants(use_all)


def sections(use_all, n):
    """[(key, offset, length)] of an arena of n blocks, in memory order; key = ("a", alpha_mode, split_alpha) for the 8 alpha
    sections of 2n bytes, ("c", colour_mode, variant, split_colour) for the 12 / 24 colour sections of 4n bytes behind them"""
    out, at = [], 0
    for am in range(4):
        for sa in (0, 1):
            out.append((("a", am, sa), at, 2 * n))
            at += 2 * n
    for cm in range(3):
        for v in range(variants(use_all)):
            for sc in (0, 1):
                out.append((("c", cm, v, sc), at, 4 * n))
                at += 4 * n
    return out


def arena_bytes(use_all, n):
    return (112 if use_all else 64) * n


def alpha_index(am, sa):
    return 2 * am + sa


def colour_index(use_all, cm, v, sc):
    return ALPHA_SECTIONS + cm * 2 * variants(use_all) + 2 * v + sc


def candidates(use_all):
    """[(alpha_mode, colour_mode, variant, split_alpha, split_colour)] in candidate order:
    candidate index = (alpha_mode * 3 + colour_mode) * order_len + position in BC3's test order"""
    return [(am, cm, v, sa, sc) for am in range(4) for cm in range(3) for v, sa, sc in oracle_auto.test_order("bc3", use_all)]


def fold(use_all, sizes, failed=()):
    """(choice, totals) of the pick over `sizes` in section order: wrapping sums in candidate order, strict `<` against
    (None, None, Variant1, split alpha, split colour) with the maximum size.  failed: the sections whose estimate failed -- every
    candidate that uses one is skipped"""
    best, best_size, totals = (0, 0, 1, 1, 1), U64_MAX, []
    for am, cm, v, sa, sc in candidates(use_all):
        total = (sizes[alpha_index(am, sa)] + sizes[colour_index(use_all, cm, v, sc)]) % U64
        totals.append(total)
        if alpha_index(am, sa) in failed or colour_index(use_all, cm, v, sc) in failed:
            continue
        if total < best_size:
            best_size, best = total, (am, cm, v, sa, sc)
    return best, totals


# ---- the statements ---------------------------------------------------------------------------------------------------------------
def alpha_values(a0, a1):
    """the eight alpha values of a BC3 alpha half, from the format's definition"""
    if a0 > a1:
        return [a0, a1] + [((8 - i) * a0 + (i - 1) * a1) // 7 for i in range(2, 8)]
    return [a0, a1] + [((6 - i) * a0 + (i - 1) * a1) // 5 for i in range(2, 6)] + [0, 255]


def alpha_uniform(w0, w1):
    """per block: whether the sixteen decoded alpha values are equal -- from the decoded values, not from the library's shortcut"""
    out = np.zeros(w0.size, dtype=bool)
    for b, (lo, hi) in enumerate(zip(w0.tolist(), w1.tolist())):
        table = alpha_values(lo & 255, (lo >> 8) & 255)
        bits = (lo >> 16) | (hi << 16)
        out[b] = len({table[(bits >> (3 * p)) & 7] for p in range(16)}) == 1
    return out


def any_normalizable(x):
    v = np.ascontiguousarray(x).view("<u4").reshape(-1, 4)
    return bool(alpha_uniform(v[:, 0], v[:, 1]).any() or A.bc2_solid(v[:, 2], v[:, 3]).any())


def section_bytes(use_all, x):
    """{key: bytes} of every section of sections(): an alpha section is the alpha endpoint part [0, 2N) of
    transform_bc3(normalize_bc3_blocks(x, alpha_mode, None), None, split_alpha, unsplit), a colour section the colour endpoint part
    [len / 2, len / 2 + 4N) of transform_bc3(normalize_bc3_blocks(x, None, colour_mode), variant, unsplit, split_colour)"""
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    n = x.size // 16
    out = {}
    alpha = [oracle_c.normalize_bc3_blocks(x, am, 0) for am in range(4)]
    colour = [oracle_c.normalize_bc3_blocks(x, 0, cm) for cm in range(3)]
    for key, _off, _len in sections(use_all, n):
        if key[0] == "a":
            out[key] = oracle_c.transform("bc3", alpha[key[1]], 0, split_colour=False, split_alpha=bool(key[2]))[:2 * n]
        else:
            out[key] = oracle_c.transform("bc3", colour[key[1]], key[2], split_colour=bool(key[3]), split_alpha=False)[x.size // 2:x.size // 2 + 4 * n]
    return out


def arena_statement(use_all, x):
    secs = section_bytes(use_all, x)
    n = np.asarray(x).size // 16
    out = np.concatenate([secs[key] for key, _off, _len in sections(use_all, n)]) if n else np.zeros(0, dtype=np.uint8)
    assert out.size == arena_bytes(use_all, n)
    return out


def literal_totals(use_all, x, estimate=R.estimate):
    """the definition read literally: one full normalise + transform per candidate, est(T[0, 2N)) + est(T[len / 2, + 4N))"""
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    n = x.size // 16
    normalized = {(am, cm): oracle_c.normalize_bc3_blocks(x, am, cm) for am in range(4) for cm in range(3)}
    totals = []
    for am, cm, v, sa, sc in candidates(use_all):
        t = oracle_c.transform("bc3", normalized[am, cm], v, split_colour=bool(sc), split_alpha=bool(sa))
        totals.append((int(estimate(t[:2 * n])) + int(estimate(t[x.size // 2:x.size // 2 + 4 * n]))) % U64)
    return totals


def section_sizes(use_all, x, estimate=R.estimate):
    secs = section_bytes(use_all, x)
    return [int(estimate(secs[key])) for key, _off, _len in sections(use_all, np.asarray(x).size // 16)]


def call_statement(use_all, x, estimate=R.estimate):
    """((alpha_mode, colour_mode, variant, split_alpha, split_colour), output bytes, totals in candidate order, any) of the whole
    call.  any == 0: the plain auto statement with its 8 / 16 totals.  Otherwise the totals are the sums over the section estimates
    (test_auto_normalize_bc3_plan.py holds them equal to literal_totals)."""
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    if not any_normalizable(x):
        sizes = []

        def recording(buf):
            sizes.append(int(estimate(buf)))
            return sizes[-1]

        (v, sa, sc), out, _calls = oracle_auto.transform_auto("bc3", x, recording, use_all)
        totals = [(a + c) % U64 for a, c in zip(sizes[0::2], sizes[1::2])]
        return (0, 0, int(v), int(sa), int(sc)), np.asarray(out), totals, False
    best, totals = fold(use_all, section_sizes(use_all, x, estimate))
    am, cm, v, sa, sc = best
    out = oracle_c.transform("bc3", oracle_c.normalize_bc3_blocks(x, am, cm), v, split_colour=bool(sc), split_alpha=bool(sa))
    return best, np.asarray(out), totals, True


# ---- the data ---------------------------------------------------------------------------------------------------------------------
ALPHA_CYCLE = 25        # odd and coprime to auto_normalize_ref.CYCLE (13): every pair of an alpha class and a colour class occurs
# data kind -> (alpha kind, colour kind)
KINDS = {"none": ("none", "none"), "cycle": ("cycle", "cycle"), "opaque": ("opaque", "none"), "zero": ("zero", "none"),
         "uniform": ("uniform", "none"), "unchanged": ("unchanged", "none"), "color0": ("none", "color0")}
ALPHA_CLASSES = {"cycle": list(range(ALPHA_CYCLE)),
                 "none": [0, 18, 24],                       # no uniform alpha half
                 # The estimator counts the positions whose 4-gram is not the first of its hash slot in the window: it sees how many
                 # DISTINCT grams a section has, not how they are mixed.  So a mode wins where it alone leaves one pair value:
                 "opaque": [26, 29, 27, 29, 28, 21],        # opaque uniform blocks among unchanged (255, 255) blocks: OpaqueFillAll
                 "zero": [26, 30, 27, 30, 28, 22],          # ... among unchanged (0, 0) blocks: OpaqueZeroAlphaMaxIndices
                 # no opaque block: modes 1, 2 and 3 write the same bytes, fewer pair values than None; the first of them wins
                 "uniform": [31, 23, 32, 23, 17, 23],
                 "unchanged": [0, 23, 24, 23, 18]}          # only blocks no alpha mode changes: four equal sections, None wins


def alpha_class_of(kind, b):
    classes = ALPHA_CLASSES[kind]
    return classes[(b + 1) % len(classes)]      # block 0 of every kind but "none" is a block some mode handles


def alpha_half(k, rng, p):
    """(a0, a1, sixteen 3-bit indices as one 48-bit number) of alpha class k; p: a palette value in 8..247
       0      non-uniform, far endpoints a0 > a1 + 7            24     non-uniform, a0 < a1 - 5, a0 != 0, a1 != 255
       1-8    all indices k - 1 = 0..7, a0 > a1                 9-16   all indices k - 9 = 0..7, a0 < a1 (index 6: 0, index 7: 255)
       17     a0 == a1 with mixed indices 0..5: uniform by the walk
       18     neighbouring endpoints (a0 == a1 + 1), indices 0 and 1: the walk answers no
       19     a0 == 0, a1 - a0 >= 5, indices 0 and 6: both 0         20     a1 == 255, a1 - a0 >= 5, indices 1 and 7: both 255
       21     unchanged (255, 255), every index 7 (eight 0xFF bytes)  22     unchanged (0, 0), every index 7      23     unchanged (p, 0), indices 0
       26-28  opaque by an index with a stale other endpoint: (255, r) index 0; (r, 255) index 1; (r, s) with r <= s, index 7
       31, 32 uniform and not opaque by an index with a stale other endpoint: (p, r) with r < p, index 0; (r, p) with r < p, index 1
       29     (255, 255) with indices 0 and 6 (255 and 0): not uniform, no mode changes it      30     (0, 0) with indices 0 and 7"""
    same = lambda i: i * 0x249249249249
    mixed = int(rng.integers(0, 1 << 48))
    two = lambda i, j: sum((i if (mixed >> q) & 1 else j) << (3 * q) for q in range(16)) & ~0x3F | i | (j << 3)   # both values occur
    far = int(rng.integers(8, 100))
    stale = int(rng.integers(0, 255))
    gap = 8 + p % 7 * 13                                             # the unchanged classes take their endpoints from the palette alone
    if k == 0:
        return min(255, p + gap), p - 8, (mixed & ~0x3F) | 0x08      # pixel 0 has index 0, pixel 1 index 1
    if k == 24:
        return max(1, p - gap), min(254, p + 6), (mixed & ~0x3F) | 0x08
    if 1 <= k <= 8:
        return min(255, p + far), p, same(k - 1)
    if 9 <= k <= 16:
        return p, min(255, p + far), same(k - 9)
    if k == 17:
        idx = sum(((mixed >> (3 * q)) & 7) % 6 << (3 * q) for q in range(16))
        return p, p, (idx & ~0x3F) | 0x08
    if k == 18:
        return p + 1, p, two(0, 1)
    if k == 19:
        return 0, p, two(0, 6)
    if k == 20:
        return min(p, 250), 255, two(1, 7)
    if k == 21:
        return 255, 255, same(7)
    if k == 22:
        return 0, 0, same(7)
    if k == 23:
        return p, 0, 0
    if k == 31:
        return p, int(rng.integers(0, p)), 0
    if k == 32:
        return int(rng.integers(0, p)), p, same(1)
    if k == 29:
        return 255, 255, two(0, 6)
    if k == 30:
        return 0, 0, two(0, 7)
    if k == 26:
        return 255, stale, 0
    if k == 27:
        return stale, 255, same(1)
    return min(stale, p), max(stale, p), same(7)


def color0_halves(n, rng):
    """colour halves on which Color0Only wins: unchanged (p, 0) blocks with mixed indices, and solid blocks by index 0 whose c1 is
    whatever the encoder left there"""
    palette = rng.integers(1, 0xFFFF, 48, dtype=np.uint32)
    colours, indices = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for b in range(n):
        p = int(palette[(b // 5) % 48])
        if b % 3 == 1:
            colours[b], indices[b] = p, (int(rng.integers(0, 1 << 32)) & ~0xF) | 0x4
        else:
            colours[b], indices[b] = p | (int(rng.integers(0, 0x10000)) << 16), 0
    return colours, indices


def blocks(kind, n, seed=0):
    """n BC3 blocks of `kind` (KINDS): the alpha halves run through the classes of alpha_half in every slot, the colour halves are
    those of auto_normalize_ref.blocks(2, ...) or color0_halves.  Alpha endpoints come from a small palette that changes every five
    blocks, so that the sections have grams for the estimator to find."""
    alpha_kind, colour_kind = KINDS[kind]
    rng = np.random.default_rng([0xA0703, list(KINDS).index(kind), n, seed])
    if colour_kind == "color0":
        colours, indices = color0_halves(n, rng)
    else:
        v = np.ascontiguousarray(A.blocks(2, colour_kind, n, seed)).view("<u4").reshape(-1, 4)
        colours, indices = v[:, 2], v[:, 3]
    palette = rng.integers(8, 248, 16)
    w0, w1 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for b in range(n):
        a0, a1, idx = alpha_half(alpha_class_of(alpha_kind, b), rng, int(palette[(b // 5) % 16]))
        assert 0 <= a0 <= 255 and 0 <= a1 <= 255 and 0 <= idx < 1 << 48
        w0[b], w1[b] = a0 | (a1 << 8) | ((idx & 0xFFFF) << 16), idx >> 16
    out = np.ascontiguousarray(np.stack([w0, w1, colours, indices], axis=1).astype("<u4")).view(np.uint8).reshape(-1)
    assert out.size == 16 * n
    return out


_CASES = {}


def case(kind, n, use_all):
    """(blocks, call statement), read-only, computed once per session"""
    key = (kind, n, use_all)
    if key not in _CASES:
        x = blocks(kind, n)
        x.setflags(write=False)
        _CASES[key] = (x, call_statement(use_all, x))
    return _CASES[key]


_ARENAS = {}


def arena_case(use_all, n):
    key = (use_all, n)
    if key not in _ARENAS:
        x = blocks("cycle", n, seed=1)
        want = arena_statement(use_all, x)
        x.setflags(write=False)
        want.setflags(write=False)
        _ARENAS[key] = (x, want)
    return _ARENAS[key]


# ---- the library ------------------------------------------------------------------------------------------------------------------
def load(pkg):
    """the library with every symbol these tests call declared: a missing symbol raises AttributeError here, a failure"""
    l = A.load(pkg)
    vp, sz, i32, u64, b = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64, C.c_bool
    u8p, bp, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_bool), C.POINTER(u64)
    l.dxtlt_transform_bc3_auto_with_normalization_device.argtypes = [vp, vp, sz, b, vp, u8p, u8p, u8p, bp, bp]
    l.dxtlt_transform_bc3_auto_with_normalization_device.restype = i32
    l.dxtlt_transform_bc3_auto_with_normalization.argtypes = [vp, vp, sz, vp, b, u8p, u8p, u8p, bp, bp, C.POINTER(C.c_uint32)]
    l.dxtlt_transform_bc3_auto_with_normalization.restype = i32
    l.dxtlt_transform_bc3_auto_device.argtypes, l.dxtlt_transform_bc3_auto_device.restype = [vp, vp, sz, b, vp, u8p, bp, bp], i32
    l.dxtlt_debug_bc3_auto_normalization_sections.argtypes = [b, u64, u64p, u64p]
    l.dxtlt_debug_bc3_auto_normalization_sections.restype = i32
    l.dxtlt_debug_bc3_auto_normalization_pick.argtypes = [b, u64p, i32, u64p, i32, u8p, u8p, u8p, bp, bp]
    l.dxtlt_debug_bc3_auto_normalization_pick.restype = i32
    l.dxtlt_debug_bc3_auto_normalization_candidates_into_device.argtypes = [b, vp, sz, vp, u64, vp]
    l.dxtlt_debug_bc3_auto_normalization_candidates_into_device.restype = i32
    return l


class Outs:
    """the five out-parameters of a call, preset to values no call writes"""

    def __init__(self):
        self.alpha, self.norm, self.mode = C.c_uint8(0xEE), C.c_uint8(0xEE), C.c_uint8(0xEE)
        self.split_alpha, self.split_colour = C.c_bool(False), C.c_bool(False)

    def refs(self):
        return C.byref(self.alpha), C.byref(self.norm), C.byref(self.mode), C.byref(self.split_alpha), C.byref(self.split_colour)

    def choice(self):
        return self.alpha.value, self.norm.value, self.mode.value, int(self.split_alpha.value), int(self.split_colour.value)

    def untouched(self):
        return self.choice() == (0xEE, 0xEE, 0xEE, 0, 0)


def last_totals(lib):
    out = (C.c_uint64 * MAX_CANDIDATES)()
    n = lib.dxtlt_debug_auto_last_totals(out, MAX_CANDIDATES)
    assert n <= MAX_CANDIDATES
    return list(out[:n])


def pick(lib, use_all, sizes):
    """(status, choice, totals) of dxtlt_debug_bc3_auto_normalization_pick"""
    n = len(sizes)
    arr, totals = (C.c_uint64 * max(1, n))(*sizes), (C.c_uint64 * MAX_CANDIDATES)()
    outs = Outs()
    rc = lib.dxtlt_debug_bc3_auto_normalization_pick(use_all, arr, n, totals, MAX_CANDIDATES, *outs.refs())
    return rc, outs.choice(), list(totals[:len(candidates(use_all))]) if rc == OK else None
