"""ctypes view of the batched auto transform (DxtltBatchAutoItem and the dxtlt_debug_*batch_auto* hooks of
include/dxtlt_estimator.h) for tests/test_batch_auto_plan.py and tests/test_batch_auto_gpu.py."""
import ctypes as C

FMT_ID = {"bc1": 1, "bc2": 2, "bc3": 3, "bc4": 4, "bc5": 5}
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16, "bc4": 8, "bc5": 16}
WINDOW = 32768


class Item(C.Structure):
    _fields_ = [("d_input", C.c_void_p), ("d_output", C.c_void_p), ("len", C.c_uint64), ("format", C.c_uint8),
                ("use_all_decorrelation_modes", C.c_uint8), ("decorrelation_mode", C.c_uint8),
                ("split_alpha_endpoints", C.c_uint8), ("split_colour_endpoints", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class PlanSection(C.Structure):
    _fields_ = [("arena_offset", C.c_uint64), ("len", C.c_uint64), ("counter", C.c_uint32), ("reserved", C.c_uint32)]


class PlanItem(C.Structure):
    _fields_ = [("chunk", C.c_uint32), ("section_count", C.c_uint32), ("arena_offset", C.c_uint64), ("arena_bytes", C.c_uint64),
                ("sections", PlanSection * 10)]


class PlanChunk(C.Structure):
    _fields_ = [("first_item", C.c_uint64), ("item_count", C.c_uint64), ("arena_bytes", C.c_uint64),
                ("candidate_launches", C.c_uint32), ("estimator_workgroups", C.c_uint32)]


def load(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    sz, vp, i32, u64p = C.c_size_t, C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)
    l.dxtlt_transform_batch_auto_device.argtypes, l.dxtlt_transform_batch_auto_device.restype = [C.POINTER(Item), sz, vp], i32
    l.dxtlt_debug_plan_batch_auto.argtypes = [C.POINTER(Item), sz, C.POINTER(PlanItem), C.POINTER(PlanChunk), sz, C.POINTER(sz)]
    l.dxtlt_debug_plan_batch_auto.restype = i32
    l.dxtlt_debug_batch_auto_last.argtypes, l.dxtlt_debug_batch_auto_last.restype = [u64p], None
    l.dxtlt_debug_batch_auto_last_totals.argtypes, l.dxtlt_debug_batch_auto_last_totals.restype = [sz, u64p, i32], i32
    l.dxtlt_debug_batch_auto_arena_cap.argtypes, l.dxtlt_debug_batch_auto_arena_cap.restype = [C.c_uint64], None
    l.dxtlt_debug_auto_last_estimation.argtypes, l.dxtlt_debug_auto_last_estimation.restype = [u64p, u64p], None
    l.dxtlt_last_error.restype = C.c_char_p
    return l


def make_items(specs):
    """specs: (fmt, input address, output address, len, use_all)"""
    arr = (Item * max(1, len(specs)))()
    for a, (fmt, src, dst, n, use_all) in zip(arr, specs):
        a.d_input, a.d_output, a.len = src, dst, n
        a.format, a.use_all_decorrelation_modes = FMT_ID.get(fmt, fmt if isinstance(fmt, int) else 0), int(bool(use_all))
        a.decorrelation_mode = a.split_alpha_endpoints = a.split_colour_endpoints = 0xEE
    return arr


def shown_lengths(fmt, n, use_all):
    """lengths of the DISTINCT sections the candidates of (fmt, use_all) show the estimator for n bytes, in slice order: what
    auto_sections (csrc/auto_launch.h) lists: the arena of the single-buffer path and a batch item's slice"""
    blocks = n // BLOCK[fmt]
    variants = 4 if use_all else 2
    if fmt == "bc1":
        return [n // 2] * (2 * variants)
    if fmt == "bc2":
        return [n // 4] * (2 * variants)
    if fmt == "bc3":
        return [blocks * 2] * 2 + [blocks * 4] * (2 * variants)
    return [blocks * 2] * (2 if fmt == "bc4" else 4)


def auto_input(fmt, blocks, style, seed):
    """`blocks` blocks whose endpoint sections have structure for the estimator to find (uniform random blocks make every
    candidate estimate alike and would test only the tie-break), in four styles that favour different settings:
      0  endpoints that repeat for a few blocks, byte k of them a multiple of the same counter (tests/test_estimator_gpu.py)
      1  the first endpoint of every pair from a palette of 5, the second random: splitting the endpoints pays
      2  pairs from a palette of 6 whole pairs: keeping the pairs together pays
      3  grey-ish RGB565 endpoints, g = r = b up to one step, c1 = c0 + 1 step: decorrelation pays
    BC2 / BC3 colour endpoints follow the same style as the leading endpoint bytes."""
    import numpy as np

    B = BLOCK[fmt]
    rng = np.random.default_rng(seed * 1315423911 % (1 << 32) + blocks * 7 + style)
    x = rng.integers(0, 256, (blocks, B), dtype=np.uint8)
    n = blocks
    if n == 0:
        return x.reshape(-1)

    def fill(cols):
        w = len(cols)
        if style == 0:
            v = (np.arange(n)[:, None] // (5 + seed % 4) + np.arange(w)[None, :] * 3) & 0xFF
        elif style == 1:
            v = rng.integers(0, 256, (n, w))
            pal = rng.integers(0, 256, (5, w // 2))
            v[:, :w // 2] = pal[rng.integers(0, 5, n)]
        elif style == 2:
            pal = rng.integers(0, 256, (6, w))
            v = pal[rng.integers(0, 6, n)]
        else:
            if w < 4:                                          # two one-byte endpoints: a slow ramp and its neighbour
                a = (np.arange(n) // 3) & 0xFF
                v = np.stack([a, (a + 1) & 0xFF], axis=1)
            else:
                l = rng.integers(0, 31, n)
                c0 = (l << 11) | ((2 * l + rng.integers(0, 2, n)) << 5) | l
                c1 = ((l + 1) << 11) | ((2 * l + 2) << 5) | (l + 1)
                v = np.stack([c0 & 0xFF, c0 >> 8, c1 & 0xFF, c1 >> 8], axis=1)
        x[:, cols] = v.astype(np.uint8)

    if fmt == "bc1":
        fill([0, 1, 2, 3])
    elif fmt == "bc2":
        fill([8, 9, 10, 11])
    elif fmt == "bc3":
        fill([0, 1])
        fill([8, 9, 10, 11])
    elif fmt == "bc4":
        fill([0, 1])
    else:
        fill([0, 1])
        fill([8, 9])
    return x.reshape(-1)
