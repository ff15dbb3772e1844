"""What the tests of the normalising batch calls share (include/dxtlt_batch_normalize.h): the C item, the bound library, the
settings and mode lists, and data with its CPU statement -- oracle.transform(fmt, oracle.normalize_bcN_blocks(x, modes), settings).

Data: BC2 / BC3 from tests/test_normalize_fused_bc23.py (blocks_of: counts below 64 start at a block every mode pair treats
differently), BC1 from the pool of tests/test_normalize_alignment.py, read the same way (`bc1_blocks`)."""
import ctypes as C

import numpy as np

import test_normalize_alignment as NA
import test_normalize_fused_bc23 as F23
from test_alignment_sweep import ALL_OFF, DEFAULT, SETTINGS  # noqa: F401

FMT_ID = {"bc1": 1, "bc2": 2, "bc3": 3}
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16}
FORMATS = ("bc1", "bc2", "bc3")
# (alpha mode, colour mode) with a mode set: 2 for BC1 and BC2, 11 for BC3
MODE_PAIRS = {"bc1": [(0, 1), (0, 2)], "bc2": [(0, 1), (0, 2)], "bc3": [(a, c) for a in range(4) for c in range(3) if (a, c) != (0, 0)]}
OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
PLAIN, SINGLE, NORMALIZING = 1, 2, 4          # DxtltDebugBatchLaunch::kind


def tile_blocks(fmt, s):
    """blocks of a tile of the batch launch: 256 lanes of 16 bytes; BC1 without the colour split runs 128-lane tiles"""
    return 256 if fmt != "bc1" else 512 if s[2] else 256


def settings_code(fmt, s):
    """variant << 2 | split_alpha << 1 | split_colour of the format's effective settings (BC3 alone has an alpha split)"""
    return (s[0] << 2) | ((1 if fmt == "bc3" and s[1] else 0) << 1) | (1 if s[2] else 0)


class Item(C.Structure):   # DxtltBatchNormalizeItem
    _fields_ = [("d_input", C.c_void_p), ("d_output", C.c_void_p), ("len", C.c_uint64), ("format", C.c_uint8),
                ("alpha_mode", C.c_uint8), ("color_mode", C.c_uint8), ("decorrelation_mode", C.c_uint8),
                ("split_alpha_endpoints", C.c_uint8), ("split_colour_endpoints", C.c_uint8), ("reserved", C.c_uint8 * 2)]


def item(fmt, src, dst, nbytes, modes, s):
    return Item(src, dst, nbytes, FMT_ID[fmt], modes[0], modes[1], s[0], s[1], s[2])


def array(items):
    return (Item * max(1, len(items)))(*items)


def bind(pkg):
    """the library with the new calls' prototypes; fails where the calls do not exist"""
    from test_batch_call_plan import Launch

    l = C.CDLL(pkg._lib.lib_path())
    items, sz, vp = C.POINTER(Item), C.c_size_t, C.c_void_p
    l.dxtlt_transform_batch_with_normalize_blocks_device.argtypes = [items, sz, vp]
    l.dxtlt_batch_any_normalizable_device.argtypes = [items, sz, vp, vp]
    l.dxtlt_debug_plan_batch_normalize_call.argtypes = [items, sz, C.POINTER(Launch), sz, C.POINTER(C.c_uint64)]
    for name in ("dxtlt_transform_batch_with_normalize_blocks_device", "dxtlt_batch_any_normalizable_device",
                 "dxtlt_debug_plan_batch_normalize_call"):
        getattr(l, name).restype = C.c_int32
    l.dxtlt_last_error.restype = C.c_char_p
    l.Launch = Launch
    return l


# ------------------------------------------------------------------------------------------------------------
# data and expectations, computed once and read-only
# ------------------------------------------------------------------------------------------------------------
_BC1, _NORM, _WANT = {}, {}, {}


def normalize(oracle, fmt, x, modes):
    if fmt == "bc1":
        return oracle.normalize_bc1_blocks(x, modes[1])
    return oracle.normalize_bc2_blocks(x, modes[1]) if fmt == "bc2" else oracle.normalize_bc3_blocks(x, modes[0], modes[1])


def bc1_blocks(oracle, n):
    """n BC1 blocks of test_normalize_alignment's pool; counts below 64 start at a block both colour modes rewrite, differently"""
    if n not in _BC1:
        pool, _ = NA.pool(oracle, "bc1")
        first = 32 * (n % NA.RUNS)
        if n < 64:
            def told_apart(i):
                b = pool[8 * i:8 * i + 8]
                return len({b.tobytes(), normalize(oracle, "bc1", b, (0, 1)).tobytes(), normalize(oracle, "bc1", b, (0, 2)).tobytes()}) == 3
            first = next(i for i in range(first, pool.size // 8 - n) if told_apart(i))
        x = pool[8 * first:8 * (first + n)].copy()
        assert x.size == 8 * n
        x.setflags(write=False)
        _BC1[n] = x
    return _BC1[n]


def blocks_of(oracle, fmt, n):
    return bc1_blocks(oracle, n) if fmt == "bc1" else F23.blocks_of(oracle, fmt, n)


def normalized(oracle, fmt, n, modes):
    modes = (modes[0] if fmt == "bc3" else 0, modes[1])
    key = (fmt, n, modes)
    if key not in _NORM:
        x = blocks_of(oracle, fmt, n)
        y = x if modes == (0, 0) else normalize(oracle, fmt, x, modes)
        y.setflags(write=False)
        _NORM[key] = y
    return _NORM[key]


def expected(oracle, fmt, s, n, modes):
    """oracle.transform(fmt, oracle.normalize_bcN_blocks(blocks_of(fmt, n), modes), settings)"""
    modes = (modes[0] if fmt == "bc3" else 0, modes[1])
    key = (fmt, s, n, modes)
    if key not in _WANT:
        w = np.ascontiguousarray(oracle.transform(fmt, normalized(oracle, fmt, n, modes), s[0], bool(s[2]), bool(s[1])))
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def modes_change_the_data(oracle, fmt, n, modes):
    return not np.array_equal(normalized(oracle, fmt, n, modes), blocks_of(oracle, fmt, n))
