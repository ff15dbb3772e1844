"""What the tests of the block formats' candidate kernels share (tests/test_auto_candidates_gpu.py, tests/test_auto_candidates_cases.py):
the STATEMENT of a candidate arena or slice -- every section of csrc/auto_launch.h's auto_sections, cut from the CPU transforms the
suite already trusts -- the one comparison, the ctypes view of the two hooks (include/dxtlt_estimator.h:
dxtlt_debug_auto_candidates_into_device, dxtlt_debug_batch_auto_candidates_device) and the case lists of the GPU tests, built here
so that the no-device test can count what they reach."""
from __future__ import annotations

import ctypes as C

import numpy as np

import batch_auto_util as BU
import bc45_ref

FMT = {1: "bc1", 2: "bc2", 3: "bc3", 4: "bc4", 5: "bc5"}
BLOCK = {1: 8, 2: 16, 3: 16, 4: 8, 5: 16}
GROUPS = [(1, False), (1, True), (2, False), (2, True), (3, False), (3, True), (4, False), (5, False)]   # the batched instantiations
SINGLE_GROUPS = GROUPS[:6]                                                                                # auto_candidates_kernel's
FILL = 0xEE
GUARD = 256
WINDOW = 32768
OK, E_LENGTH, E_ARGUMENT = 0, 1, 2


# ---- the layout: auto_sections ----------------------------------------------------------------------------------------------------
def sections(fmt, use_all, n):
    """[(name, offset, length, bytes per block)] of a slice of n blocks, in memory order"""
    names = []
    if fmt == 4:
        names = [("endpoint pairs", 2), ("endpoints split", 2)]
    elif fmt == 5:
        names = [("red pairs", 2), ("red split", 2), ("green pairs", 2), ("green split", 2)]
    else:
        if fmt == 3:
            names = [("alpha pairs", 2), ("alpha split", 2)]
        for v in range(4 if use_all else 2):
            names += [(f"colour pairs, variant {v}", 4), (f"colour split, variant {v}", 4)]
    out, at = [], 0
    for name, per in names:
        out.append((name, at, per * n, per))
        at += per * n
    return out


def slice_bytes(fmt, use_all, n):
    return sum(s[2] for s in sections(fmt, use_all, n))


def workgroup_blocks(fmt):
    """W: the blocks of a 256-lane workgroup, one 16-byte vector per lane"""
    return 512 if fmt in (1, 4) else 256


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def statement(oracle, fmt, use_all, x):
    """the expected slice of (fmt, use_all) for the AoS blocks `x`, section by section in auto_sections order"""
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    n = x.size // BLOCK[fmt]
    name = FMT[fmt]
    parts = []
    if fmt in (4, 5):
        pairs, split = bc45_ref.transform(name, x, False), bc45_ref.transform(name, x, True)
        for a, b in bc45_ref.endpoint_sections(name, n):
            parts += [pairs[a:b], split[a:b]]
    else:
        if fmt == 3:
            parts += [oracle.transform("bc3", x, 0, False, split_alpha=sa)[:2 * n] for sa in (False, True)]
        at = 0 if fmt == 1 else 8 * n
        for v in range(4 if use_all else 2):
            parts += [oracle.transform(name, x, v, split_colour=sc)[at:at + 4 * n] for sc in (False, True)]
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    assert [p.size for p in parts] == [s[2] for s in sections(fmt, use_all, n)] and out.size == slice_bytes(fmt, use_all, n)
    return out


_INPUTS = {}


def random_input(oracle, fmt, use_all, n, seed=0):
    """(blocks, their statement), both read-only, computed once: uniform random bytes, so that a byte in a wrong place is a wrong byte"""
    key = (fmt, use_all, n, seed)
    if key not in _INPUTS:
        x = np.random.default_rng([0xA07C, fmt, int(use_all), n, seed]).integers(0, 256, n * BLOCK[fmt], dtype=np.uint8)
        want = statement(oracle, fmt, use_all, x)
        x.setflags(write=False)
        want.setflags(write=False)
        _INPUTS[key] = (x, want)
    return _INPUTS[key]


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def where(fmt, use_all, n, i):
    """byte i of a slice in words: its section, the byte inside it and the block it belongs to"""
    for name, off, length, per in sections(fmt, use_all, n):
        if off <= i < off + length:
            o = i - off
            if "split" not in name:
                block = o // per
            elif per == 4:
                block = (o % (2 * n)) // 2          # all c0, then all c1: two bytes per block each
            else:
                block = o % n                       # all first endpoints, then all second: one byte per block each
            return f"section '{name}' byte {o} (block {block})"
    return "behind the slice"


def differences(got, placed, fill=FILL):
    """THE comparison.  placed: [(offset, expected slice, (fmt, use_all, n), tag)], disjoint.  [] when every slice of `got` equals its
    statement and every other byte holds `fill`; else one line per slice that differs -- the section, block and byte of the first
    wrong byte -- and one for the bytes written outside every slice."""
    image, covered = np.full(got.size, fill, dtype=np.uint8), np.zeros(got.size, dtype=bool)
    for off, want, _shape, tag in placed:
        assert 0 <= off and off + want.size <= got.size and not covered[off:off + want.size].any(), tag
        image[off:off + want.size] = want
        covered[off:off + want.size] = True
    if np.array_equal(got, image):
        return []
    out = []
    for off, want, (fmt, use_all, n), tag in placed:
        bad = np.nonzero(got[off:off + want.size] != want)[0]
        if bad.size:
            i = int(bad[0])
            out.append(f"{tag}: {bad.size} of {want.size} bytes differ, first at slice byte {i}, {where(fmt, use_all, n, i)}: "
                       f"got {int(got[off + i])}, want {int(want[i])}")
    stray = np.nonzero((got != fill) & ~covered)[0]
    if stray.size:
        out.append(f"{stray.size} bytes outside every slice were written, first at {int(stray[0])}")
    return out


# ---- the library ------------------------------------------------------------------------------------------------------------------
def load(pkg):
    """the library with every symbol these tests call declared: a missing symbol raises AttributeError here, a failure"""
    l = BU.load(pkg)
    vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64
    l.dxtlt_debug_auto_candidates_into_device.argtypes = [i32, C.c_bool, vp, sz, vp, u64, vp]
    l.dxtlt_debug_auto_candidates_into_device.restype = i32
    l.dxtlt_debug_batch_auto_candidates_device.argtypes = [C.POINTER(BU.Item), sz, sz, vp, u64, vp]
    l.dxtlt_debug_batch_auto_candidates_device.restype = i32
    l.dxtlt_debug_auto_last_totals.argtypes, l.dxtlt_debug_auto_last_totals.restype = [C.POINTER(u64), i32], i32
    return l


def auto_plan(lib, arr, count, chunk_capacity=64):
    """(items, chunks) of dxtlt_debug_plan_batch_auto at the cap in force on the thread"""
    items, chunks, n = (BU.PlanItem * max(1, count))(), (BU.PlanChunk * chunk_capacity)(), C.c_size_t(0)
    rc = lib.dxtlt_debug_plan_batch_auto(arr, count, items, chunks, chunk_capacity, C.byref(n))
    assert rc == 0 and n.value <= chunk_capacity, (rc, n.value, lib.dxtlt_last_error())
    return list(items[:count]), list(chunks[:n.value])


# ---- the single kernel's cases ----------------------------------------------------------------------------------------------------
ARENA_RESIDUES = (0, 16, 48, 112)      # of a 128-byte line
INPUT_OFFSETS = (0, 16, 80)            # past a 256-byte boundary


def single_counts(fmt, small=True):
    """every N in 1..66 (`small`), around one and two workgroups, 4096 + r: every N mod 8"""
    w = workgroup_blocks(fmt)
    return (list(range(1, 67)) if small else []) + [w - 1, w, w + 1, 2 * w - 1, 2 * w + 1] + [4096 + r for r in range(8)]


def single_jobs(fmt, small=True):
    """[(n, input offset past a 256-byte boundary, arena residue of a 256-byte line)]: the offsets and residues in turn, 3 and 4
    being coprime every pair of them occurs; the arena's residue of a 128-byte line is ARENA_RESIDUES' and both halves of 256 occur"""
    return [(n, INPUT_OFFSETS[k % 3], ARENA_RESIDUES[k % 4] + 128 * (k // 4 % 2)) for k, n in enumerate(single_counts(fmt, small))]


def single_kernels(fmt, use_all, n):
    """the kernels launch_auto_candidates runs for n blocks"""
    vectors = n // 2 if fmt == 1 else n
    out = []
    if vectors:
        out.append(("auto_candidates_kernel", fmt, use_all))
    if fmt == 1 and n % 2:
        out.append(("auto_candidates_bc1_last_block", use_all))
    return out


# ---- every colour -------------------------------------------------------------------------------------------------------------------
def lane_pairs():
    """the (524 288, 2) colour pairs (lo, hi) of tests/test_array_ops_sweep_gpu.py: every 565 value in either half of a dword against
    0x0000, 0xFFFF, its complement and a fixed permutation of it"""
    c = np.arange(65536, dtype=np.int64)
    partners = [np.zeros_like(c), np.full_like(c, 0xFFFF), c ^ 0xFFFF, (c * 40503 + 12345) & 0xFFFF]
    lo_fixed = np.concatenate([np.stack([c, p], axis=1) for p in partners])
    hi_fixed = np.concatenate([np.stack([p, c], axis=1) for p in partners])
    return np.concatenate([lo_fixed, hi_fixed]).astype("<u2")


def every_colour_blocks(fmt):
    """BC2: one block per pair.  BC1: the pairs, then the pairs moved on by one block -- a vector holds two blocks, so every pair sits
    in its first dword once and in its third once.  Everything that is not a colour endpoint is random."""
    pairs = lane_pairs()
    if fmt == 1:
        pairs = np.concatenate([pairs, np.roll(pairs, 1, axis=0)])
    n = pairs.shape[0]
    x = np.random.default_rng(0xC010 + fmt).integers(0, 256, (n, BLOCK[fmt]), dtype=np.uint8)
    at = 0 if fmt == 1 else 8
    x[:, at:at + 4] = np.ascontiguousarray(pairs).view(np.uint8).reshape(n, 4)
    return x.reshape(-1)


def colour_dwords(fmt, x):
    """(vectors, endpoint dwords of a vector that hold colours): what a lane hands decorrelate2"""
    v = np.ascontiguousarray(x).view("<u4").reshape(-1, 4)
    return v[:, [0, 2]] if fmt == 1 else v[:, [2]]


# ---- the batched kernel's cases: (fmt, use_all, blocks, misalignment of d_input) ------------------------------------------------------
def group_misalignments(g):
    """of group g's five items: 0 (vector loads), a non-zero multiple of 4 (dword loads), an odd one (byte loads), and two more so
    that the eight groups together have every misalignment 0..15"""
    return [0, (4, 8, 12)[g % 3], 2 * g + 1, (2 * g + 2) % 16, (7 * g + 5) % 16]


def group_counts(g, small=True):
    fmt = GROUPS[g][0]
    if fmt in (1, 4):      # the half lane: the last lane of a workgroup; lane 0 of a workgroup of its own, twice; alone
        return [4096 + g, 511, 513, 1025, 1 if small else 2]
    return [1 + 9 * g if small else 255, 255, 257, 513, 4096 + g]


def cases_mixed(small=True):
    """41 items, the groups in turn so that no launch's entries are neighbours in the batch, an empty item in the middle"""
    out = []
    for j in range(5):
        for g, (fmt, use_all) in enumerate(GROUPS):
            out.append((fmt, use_all, group_counts(g, small)[j], group_misalignments(g)[j]))
    out[20:20] = [(2, True, 0, 0)]
    return out


def cases_deep():
    """300 items of one group (BC1, fast): nine steps of bisection; the half lane in every position; every misalignment"""
    counts = [1, 511, 513, 1025, 100, 2049]
    return [(1, False, counts[k % 6], k % 16) for k in range(300)]


def cases_owners():
    """three entries of three, two and three workgroups: the first, a middle and the last entry own workgroups of the launch"""
    return [(3, False, 600, 0), (3, False, 300, 4), (3, False, 513, 1)]


def cases_count(n):
    return [(2, True, 257, 0), (2, True, 66, 3)][:n]


MIXED_CHUNK_CAP = 200_000        # the mixed batch in more than three chunks; its largest slice is 4101 * 36 bytes


def load_arm(fmt, n, misalign, v):
    """how lane v of an item reads its vector (batch_auto_candidates_kernel)"""
    half = fmt in (1, 4) and n % 2 == 1 and v == n // 2
    if misalign == 0 and not half:
        return "vector"
    return "dword" if misalign % 4 == 0 else "byte"


def half_lane(fmt, n):
    """None, or where the half lane of an item lies: (workgroup, lane, lanes of that workgroup)"""
    if fmt not in (1, 4) or n % 2 == 0:
        return None
    v = n // 2
    return v // 256, v % 256, v % 256 + 1          # the half lane is the item's last lane


def bisection_steps(entries):
    """iterations of the kernel's loop over first_wg: the same for every workgroup"""
    lo, hi, steps = 0, entries - 1, 0
    while lo < hi:                                  # the longest path: always the upper half
        lo = (lo + hi + 1) >> 1
        steps += 1
    return steps


def workgroups(fmt, n):
    lanes = (n + 1) // 2 if fmt in (1, 4) else n
    return (lanes + 255) // 256


def fake_items(cases, base=0x7000_0000_0000):
    """the cases as items at made-up addresses with the cases' misalignments (the plan hook dereferences nothing)"""
    specs, at = [], base
    out_base = base + (1 << 40)
    for fmt, use_all, n, mis in cases:
        nbytes = n * BLOCK[fmt]
        specs.append((fmt, at + mis, out_base + (at - base), nbytes, use_all))
        at += (nbytes + 16 + GUARD + 255) & ~255
    return BU.make_items(specs)
