"""Case lists of the array-operation sweep (tests/test_array_ops_sweep_gpu.py): the stand-alone colour-array calls of
include/dxtlt_color565.h, and decode_blocks / count_pixel_differences of include/dxtlt_decode.h.  Pure: numpy and ctypes, no torch,
no device.  tests/test_array_ops_cases.py proves, through dxtlt_debug_plan_array_op alone, what each list reaches.

A pointer is named by its residue: the offset of its first byte from a 256-byte aligned address (pixels_gpu_common.Arena).  The
plan hook takes addresses as numbers, so a residue IS a valid address for it."""
import collections
import ctypes as C

import numpy as np

OP_YCOCG, OP_RECORRELATE_SPLIT, OP_SPLIT_ENDPOINTS, OP_DECODE, OP_DIFFERENCE = 0, 1, 2, 10, 20      # include/dxtlt_decode.h
FORMATS = ("bc1", "bc2", "bc3")
KIND = {"bc1": 1, "bc2": 2, "bc3": 3}
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16}
THREADS = 256                                          # lanes per workgroup of every kernel here (the plan reports it)


class Plan(C.Structure):                               # DxtltDebugArrayOpPlan
    _fields_ = [("vector", C.c_int32), ("threads", C.c_int32), ("vector_lanes", C.c_uint64), ("single_lanes", C.c_uint64),
                ("workgroups", C.c_uint64), ("steps", C.c_uint64)]


def declare(l):
    l.dxtlt_debug_plan_array_op.argtypes = [C.c_int32] + [C.c_uint64] * 4 + [C.POINTER(Plan)]
    l.dxtlt_debug_plan_array_op.restype = C.c_int32
    l.dxtlt_debug_array_op_slices.argtypes = [C.POINTER(C.c_uint64)] * 2
    l.dxtlt_debug_array_op_slices.restype = None
    return l


def plan(l, op, count, a0, a1=0, a2=0):
    p = Plan()
    assert l.dxtlt_debug_plan_array_op(op, a0, a1, a2, count, C.byref(p)) == 0
    assert p.threads == THREADS
    return p


def slices(l):
    """(blocks per slice of the host decode call, bytes per slice of the host difference call)"""
    blocks, nbytes = C.c_uint64(0), C.c_uint64(0)
    l.dxtlt_debug_array_op_slices(C.byref(blocks), C.byref(nbytes))
    return int(blocks.value), int(nbytes.value)


# ---- ycocg: (n colours, source residue, destination residue; destination None = in place) ------------------------------------------
YCOCG_N = 2051                                         # at (0, 0): 256 vector lanes, then 3 singles in a workgroup of their own
YCOCG_VARIANTS = (1, 2, 3)
YCOCG_COUNT_POINTERS = ((0, 0), (16, 48), (0, None))


def ycocg_offset_cases():
    """all 256 residue pairs mod 16, then the 16 in-place cases"""
    return [(YCOCG_N, s, d) for s in range(16) for d in range(16)] + [(YCOCG_N, s, None) for s in range(16)]


def ycocg_counts():
    return sorted(set(range(0, 601)) | set(range(2048 - 9, 2048 + 10)) | set(range(4096 - 9, 4096 + 10)))


def ycocg_count_cases():
    return [(n, s, d) for s, d in YCOCG_COUNT_POINTERS for n in ycocg_counts()]


def ycocg_plan(l, case):
    n, s, d = case
    return plan(l, OP_YCOCG, n, s, s if d is None else d)


# ---- recorrelate split: (pairs, src0 residue, src1 residue, dst residue), three separate buffers -----------------------------------
SPLIT_PAIRS = 1027                                     # vector route: 256 lanes of four pairs, then 3 single pairs
SPLIT_DST_RESIDUES = (0, 1, 2, 4, 8, 12, 15, 16)
SPLIT_VARIANTS = (0, 1, 2, 3)
SPLIT_COUNT_POINTERS = ((0, 0, 0), (8, 8, 16), (8, 0, 0))


def split_offset_cases():
    return [(SPLIT_PAIRS, s0, s1, d) for s0 in range(16) for s1 in range(16) for d in SPLIT_DST_RESIDUES]


def split_counts():
    return sorted(set(range(0, 301)) | set(range(1024 - 5, 1024 + 6)) | set(range(2048 - 5, 2048 + 6)))


def split_count_cases():
    return [(p, s0, s1, d) for s0, s1, d in SPLIT_COUNT_POINTERS for p in split_counts()]


def split_plan(l, case):
    pairs, s0, s1, d = case
    return plan(l, OP_RECORRELATE_SPLIT, pairs, s0, s1, d)


# ---- split endpoints: (pairs, input residue, output residue) -----------------------------------------------------------------------
ENDPOINT_PAIRS = (2056, 2051)                          # a multiple of 8 (both output halves can be aligned) and one that is not


def endpoint_offset_cases():
    return [(p, i, o) for p in ENDPOINT_PAIRS for i in range(16) for o in range(16)]


def endpoint_counts():
    return sorted(set(range(0, 301)) | set(range(2048 - 9, 2048 + 10)))


def endpoint_count_cases():
    return [(p, 0, 0) for p in endpoint_counts()]


def endpoint_plan(l, case):
    pairs, i, o = case
    return plan(l, OP_SPLIT_ENDPOINTS, pairs, i, o)


# ---- decode: (blocks, input residue, output residue), per format -------------------------------------------------------------------
DECODE_N = 259                                         # two workgroups, the second holding three blocks of one wave
DECODE_COUNT_POINTERS = ((0, 0), (8, 0), (0, 8), (1, 1))
POOL_BLOCKS = 1021                                     # prime: a tiling of the pool meets every lane and both unrolled slots


def decode_offset_cases():
    return [(DECODE_N, i, o) for i in range(17) for o in range(17)]


def decode_counts():
    return sorted(set(range(0, 131)) | set(range(256 - 3, 256 + 4)) | set(range(512 - 3, 512 + 4)))


def decode_count_cases():
    return [(n, i, o) for i, o in DECODE_COUNT_POINTERS for n in decode_counts()]


def decode_plan(l, fmt, case):
    n, i, o = case
    return plan(l, OP_DECODE + KIND[fmt], n, i, o)


def pool_window(n):
    """first block of the window of `n` pool blocks a case of n blocks decodes: it moves with n"""
    assert 0 <= n <= POOL_BLOCKS
    return (7 * n) % (POOL_BLOCKS - n + 1)


def block_pool(fmt):
    """(1021, block size) blocks from the structured families of test_decode.decode_cases, evenly drawn -- c0 == c1, c0 < c1,
    c0 > c1 with random indices; BC3: every alpha endpoint pair with an index ramp, among them 0 / 255 and 255 / 0"""
    from test_decode import decode_cases

    bs = BLOCK[fmt]
    rows = decode_cases(fmt, np.random.default_rng(0xA0 + KIND[fmt]), n_random=1).reshape(-1, bs)[1:]    # [0] is the random block
    colour, alpha = rows[:80_000], rows[80_000:]           # four families of 20 000; then (BC3) alpha pair e = a0 + 256 a1 at row e
    if fmt != "bc3":
        assert alpha.shape[0] == 0
        pick = colour[np.linspace(0, colour.shape[0] - 1, POOL_BLOCKS).astype(np.int64)]
    else:
        assert alpha.shape[0] == 65536
        a = alpha[np.concatenate([[0xFF00, 0x00FF], np.linspace(0, 65535, 419).astype(np.int64)])]
        pick = np.concatenate([colour[np.linspace(0, colour.shape[0] - 1, POOL_BLOCKS - a.shape[0]).astype(np.int64)], a])
    pick = np.ascontiguousarray(pick)
    assert pick.shape == (POOL_BLOCKS, bs)
    pick.setflags(write=False)
    return pick


def colour_words(fmt, blocks):
    """(c0, c1) of every block"""
    col = BLOCK[fmt] - 8
    b = blocks.astype(np.int64)
    return b[:, col] | b[:, col + 1] << 8, b[:, col + 2] | b[:, col + 3] << 8


# ---- difference --------------------------------------------------------------------------------------------------------------------
DIFF_STEP = 2 * THREADS                                # blocks a workgroup takes per step: two per lane
DIFF_BLOCKS = 2 * DIFF_STEP + 37                       # 1061
DIFF_POINTERS = ((0, 0), (3, 0), (0, 5), (8, 8))       # (8, 8): vector loads for BC1, byte loads for BC2 / BC3
DIFF_GRID = 4096
WALK_BLOCKS = 2 * DIFF_GRID * DIFF_STEP + DIFF_STEP + 37     # two whole passes of the grid, one more step of workgroup 0, a tail
EQUAL, EQUIVALENT, DIFFERENT = 0, 1, 2
DIFF_KINDS = (DIFFERENT, EQUIVALENT, EQUAL, DIFFERENT, EQUAL, EQUIVALENT, EQUAL)      # block i is of kind DIFF_KINDS[i % 7]


def difference_prefix_lengths():
    return list(range(1, DIFF_BLOCKS + 1))


def difference_plan(l, fmt, n, a, b):
    return plan(l, OP_DIFFERENCE + KIND[fmt], n, a, b)


def block_kinds(n):
    return np.array(DIFF_KINDS, dtype=np.int64)[np.arange(n) % 7]


def difference_pair(fmt, n, seed):
    """(a, b), n blocks each, b's block i of kind DIFF_KINDS[i % 7] against a's: byte-equal; another encoding of the same pixels
    (c0 == c1: BC1, three-colour mode, indices 0 and 1 show the same colour; BC2 / BC3: four equal palette entries, the indices
    are free); or one bit of the red field of both endpoints flipped, which changes every palette entry."""
    rng = np.random.default_rng(seed)
    bs, col = BLOCK[fmt], BLOCK[fmt] - 8
    a = rng.integers(0, 256, (n, bs), dtype=np.uint8)
    kinds = block_kinds(n)
    eq = kinds == EQUIVALENT
    a[eq, col + 2:col + 4] = a[eq, col:col + 2]
    if fmt == "bc1":
        a[eq, 4:8] = 0x55
    b = a.copy()
    if fmt == "bc1":
        b[eq, 4:8] = 0x00
    else:
        b[eq, col + 4:] = rng.integers(0, 256, (int(eq.sum()), 4), dtype=np.uint8)
        assert not (b[eq, col + 4:] == a[eq, col + 4:]).all(axis=1).any()
    df = kinds == DIFFERENT
    b[df, col + 1] ^= 0x40
    b[df, col + 3] ^= 0x40
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def solid_pair(fmt, n):
    """two arrays of n solid blocks (c0 == c1, indices 0; opaque alpha) whose blue fields differ in every block"""
    bs, col = BLOCK[fmt], BLOCK[fmt] - 8
    k = np.arange(n, dtype=np.int64)
    c = (k * 2654435761 >> 7) & 0xFFFF
    a = np.zeros((n, bs), dtype=np.uint8)
    a[:, :col] = 0xFF
    a[:, col], a[:, col + 1] = c & 255, c >> 8
    a[:, col + 2:col + 4] = a[:, col:col + 2]
    b = a.copy()
    b[:, col] ^= (1 + k % 31).astype(np.uint8)          # bits 0..4 of the low byte: the blue field
    b[:, col + 2] = b[:, col]
    return a, b
