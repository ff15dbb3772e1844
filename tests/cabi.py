"""ctypes view of the reference-shaped C APIs (include/dltbc{1,2,3}core.h, include/dltbc{1,2}.h,
include/dlt_size_estimator.h) for the tests."""
from __future__ import annotations

import ctypes as C
import zlib

MAXFN = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))
ESTFN = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))


class DltSizeEstimator(C.Structure):
    _fields_ = [("Context", C.c_void_p), ("MaxCompressedSize", MAXFN), ("EstimateCompressedSize", ESTFN)]


class CoreSettings2(C.Structure):  # Dltbc1/2TransformSettings, core layout
    _fields_ = [("SplitColourEndpoints", C.c_bool), ("DecorrelationMode", C.c_uint8)]


class CoreSettings3(C.Structure):
    _fields_ = [("SplitAlphaEndpoints", C.c_bool), ("SplitColourEndpoints", C.c_bool), ("DecorrelationMode", C.c_uint8)]


class AutoSettings(C.Structure):
    _fields_ = [("UseAllModes", C.c_bool)]


class Result(C.Structure):
    _fields_ = [("ErrorCode", C.c_int32)]


def bind(lib):
    vp, sz = C.c_void_p, C.c_size_t
    for n, S in ((1, CoreSettings2), (2, CoreSettings2), (3, CoreSettings3)):
        for d in ("transform", "untransform"):
            f = getattr(lib, f"dltbc{n}core_{d}")
            f.argtypes, f.restype = [vp, sz, vp, sz, S], Result
        f = getattr(lib, f"dltbc{n}core_transform_auto")
        f.argtypes, f.restype = [vp, sz, vp, sz, C.POINTER(DltSizeEstimator), AutoSettings, C.POINTER(S)], Result
    for n in (1, 2, 3):
        p = f"dltbc{n}_"
        getattr(lib, p + "new_ManualTransformBuilder").argtypes = []
        getattr(lib, p + "new_ManualTransformBuilder").restype = vp
        getattr(lib, p + "free_ManualTransformBuilder").argtypes = [vp]
        getattr(lib, p + "free_ManualTransformBuilder").restype = None
        getattr(lib, p + "clone_ManualTransformBuilder").argtypes = [vp]
        getattr(lib, p + "clone_ManualTransformBuilder").restype = vp
        getattr(lib, p + "ManualTransformBuilder_SetDecorrelationMode").argtypes = [vp, C.c_uint8]
        getattr(lib, p + "ManualTransformBuilder_SetDecorrelationMode").restype = None
        getattr(lib, p + "ManualTransformBuilder_SetSplitColourEndpoints").argtypes = [vp, C.c_bool]
        getattr(lib, p + "ManualTransformBuilder_SetSplitColourEndpoints").restype = None
        getattr(lib, p + "ManualTransformBuilder_ResetToDefaults").argtypes = [vp]
        getattr(lib, p + "ManualTransformBuilder_ResetToDefaults").restype = None
        for d in ("Transform", "Untransform"):
            f = getattr(lib, p + "ManualTransformBuilder_" + d)
            f.argtypes, f.restype = [vp, sz, vp, sz, vp], Result
        getattr(lib, p + "new_AutoTransformBuilder").argtypes = [C.POINTER(DltSizeEstimator)]
        getattr(lib, p + "new_AutoTransformBuilder").restype = vp
        getattr(lib, p + "free_AutoTransformBuilder").argtypes = [vp]
        getattr(lib, p + "free_AutoTransformBuilder").restype = None
        f = getattr(lib, p + "AutoTransformBuilder_SetUseAllDecorrelationModes")
        f.argtypes, f.restype = [vp, C.c_bool], Result
        f = getattr(lib, p + "AutoTransformBuilder_Transform")
        f.argtypes, f.restype = [vp, vp, sz, vp, sz, C.POINTER(vp)], Result
        f = getattr(lib, p + "error_message")
        f.argtypes, f.restype = [C.c_int32], C.c_char_p
    lib.dltbc3_ManualTransformBuilder_SetSplitAlphaEndpoints.argtypes = [vp, C.c_bool]
    lib.dltbc3_ManualTransformBuilder_SetSplitAlphaEndpoints.restype = None
    return lib


BATCH_HOST_ALONE = 0xFFFFFFFF


def plan_batch_host(lib, lens, cap):
    """dxtlt_debug_plan_batch_host (no device): how dxtlt_transform_batch_host cuts items of these lengths at a chunk cap of `cap`
    bytes.  (chunk per item -- BATCH_HOST_ALONE for one that goes out alone --, slot per item, bytes per chunk, arena bytes)"""
    u64, sz = C.c_uint64, C.c_size_t
    f = lib.dxtlt_debug_plan_batch_host
    f.argtypes = [C.POINTER(u64), sz, u64, C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64), sz, C.POINTER(u64)]
    f.restype = C.c_int32
    n = len(lens)
    arr, chunk_of, slot, arena = (u64 * max(1, n))(*lens), (C.c_uint32 * max(1, n))(), (u64 * max(1, n))(), u64(99)
    chunk_bytes = (u64 * max(1, n))()          # no more chunks than items
    chunks = f(arr, n, cap, chunk_of, slot, chunk_bytes, n, C.byref(arena))
    assert 0 <= chunks <= n
    return list(chunk_of)[:n], list(slot)[:n], list(chunk_bytes)[:chunks], arena.value


def make_estimator(kind: str, log=None):
    """kind: 'dummy' (size = len, like the reference's C dummy estimator, bc1 c_api/transform_auto.rs:200-231),
    'zlib' (zlib level 1 size), 'zstd' (the system libzstd at level 1 through tools/zstd_ratio.py: what the reference's
    estimator crate does, extensions/compressors/dxt-lossless-transform-zstd/src/lib.rs:146-200, with zstd 1.5.7),
    'fail_max' / 'fail_est' (callback errors)."""
    if kind == "zstd":
        from tools import zstd_ratio

    def py_estimate(buf: bytes) -> int:
        if kind == "zlib":
            return len(zlib.compress(buf, 1))
        if kind == "zstd":
            return zstd_ratio.compressed_size(buf, 1) if buf else 0
        if kind == "crc":          # every byte of the section matters; the log records what the estimator was shown
            return zlib.crc32(buf) & 0xFFFFF
        return len(buf)

    @MAXFN
    def max_fn(ctx, n, out):
        if kind == "fail_max":
            return 41
        out[0] = n + 64 if kind in ("zlib", "crc", "zstd") else (0 if kind == "dummy0" else n)
        return 0

    @ESTFN
    def est_fn(ctx, inp, n, scratch, scratch_len, out):
        if kind == "fail_est":
            return 42
        data = C.string_at(inp, n) if n else b""
        if log is not None:
            log.append((n, zlib.crc32(data)) if kind == "crc" else n)
        out[0] = py_estimate(data)
        return 0

    est = DltSizeEstimator(None, max_fn, est_fn)
    est._keep = (max_fn, est_fn)
    return est, py_estimate


SIZE_MAX = 2**64 - 1


class ScriptedFailure(Exception):
    """what scripted_estimate raises where the C estimator returns an error code"""

    def __init__(self, code):
        super().__init__(code)
        self.code = code


def section_key(buf):
    data = bytes(buf)
    return len(data), zlib.crc32(data)


def scripted_estimate(table, default, log=None, fail_at=None):
    """estimate(bytes_like) -> size for the CPU statements: the answer table[(len, crc32)] (or `default`), a size or
    ("fail", code), which raises ScriptedFailure(code).  fail_at = (k, code): call number k (from 0) fails whatever it shows --
    for the sequential routes, where a section several candidates share is shown several times.  log receives the keys in call
    order, the failing call's included."""
    count = [0]

    def estimate(buf):
        key = section_key(buf)
        k, count[0] = count[0], count[0] + 1
        if log is not None:
            log.append(key)
        ans = ("fail", fail_at[1]) if fail_at is not None and fail_at[0] == k else table.get(key, default)
        if isinstance(ans, tuple):
            raise ScriptedFailure(ans[1])
        return ans

    return estimate


def scripted_estimator(table, default, log=None, fail_at=None, max_extra=64):
    """A DltSizeEstimator whose answers are scripted: scripted_estimate behind the C callbacks.  A section is known by its
    (len, crc32(bytes)), not by the call's position: the parallel route estimates each distinct section once, in any order
    (list.append and the counter run under the interpreter lock).  MaxCompressedSize answers n + max_extra, or 0 (no scratch
    buffer) when max_extra is None."""
    py = scripted_estimate(table, default, log, fail_at)

    @MAXFN
    def max_fn(ctx, n, out):
        out[0] = 0 if max_extra is None else n + max_extra
        return 0

    @ESTFN
    def est_fn(ctx, inp, n, scratch, scratch_len, out):
        try:
            out[0] = py(C.string_at(inp, n) if n else b"")
        except ScriptedFailure as f:
            return f.code
        except Exception:               # a key the table does not know and no default: the call must not look like a success
            return 0xBAD
        return 0

    est = DltSizeEstimator(None, max_fn, est_fn)
    est._keep = (max_fn, est_fn)
    return est


def auto_candidates(fmt: str, use_all: bool):
    """the candidates in the order they are compared, as (mode, split_alpha, split_colour); BC4 / BC5: (0, split_endpoints, 0)"""
    from oracle import oracle_auto

    if fmt in ("bc4", "bc5"):
        return [(0, 0, 0), (0, 1, 0)]
    return list(oracle_auto.test_order(fmt, use_all))


def cpu_transform(fmt: str, x, cand):
    """the CPU statement's transform of x with a candidate of auto_candidates"""
    from oracle import oracle_c

    import bc45_ref

    if fmt in ("bc4", "bc5"):
        return bc45_ref.transform(fmt, x, bool(cand[1]))
    return oracle_c.transform(fmt, x, cand[0], cand[2], cand[1])


def candidate_sections(fmt: str, x, use_all: bool):
    """[(candidate, [(section id, key)])] for every candidate, in the order the reference tries them and shows their sections --
    BC1 [0, n/2); BC2 [n/2, 3n/4); BC3 alpha [0, 2N) then colour [n/2, n/2 + 4N); BC4 [0, 2N); BC5 [0, 2N) then [8N, 10N) --
    from the CPU statements alone.  A section id names a DISTINCT section: ("c", mode, split_colour), ("a", split_alpha),
    ("e" / "r" / "g", split_endpoints); candidates that share settings share it."""
    n = len(x)
    blocks = n // (8 if fmt in ("bc1", "bc4") else 16)
    out = []
    for cand in auto_candidates(fmt, use_all):
        mode, sa, sc = cand
        t = cpu_transform(fmt, x, cand)
        if fmt == "bc1":
            spans = [(("c", mode, sc), 0, n // 2)]
        elif fmt == "bc2":
            spans = [(("c", mode, sc), n // 2, 3 * n // 4)]
        elif fmt == "bc3":
            spans = [(("a", sa), 0, 2 * blocks), (("c", mode, sc), n // 2, n // 2 + 4 * blocks)]
        elif fmt == "bc4":
            spans = [(("e", sa), 0, 2 * blocks)]
        else:
            spans = [(("r", sa), 0, 2 * blocks), (("g", sa), 8 * blocks, 10 * blocks)]
        out.append((cand, [(sid, section_key(t[a:b])) for sid, a, b in spans]))
    return out


def distinct_sections(sections):
    """{section id: key} of candidate_sections' result; asserts the condition every scripted table rests on: a section id has one
    key, and the distinct sections of the input have pairwise different keys"""
    keys = {}
    for _cand, secs in sections:
        for sid, key in secs:
            assert keys.setdefault(sid, key) == key, sid
    assert len(set(keys.values())) == len(keys), "two distinct sections with the same (len, crc32)"
    return keys


def normalization_sections(x, use_all: bool):
    """[((norm, variant, split), key)] of transform_bc1_auto_with_normalization's 3 x 4 / 3 x 8 candidates in its order: the
    colour section [0, n/2) of the transform of each buffer of normalize_blocks_all_modes"""
    from oracle import oracle_auto, oracle_c

    outs, any_normalized = oracle_c.normalize_bc1_blocks_all_modes(x)
    assert any_normalized
    return [((norm, v, sc), section_key(oracle_c.transform("bc1", outs[norm], v, sc)[: len(x) // 2]))
            for norm in range(3) for v, _sa, sc in oracle_auto.test_order("bc1", use_all)]


def zstd_c_estimator(level: int = 1):
    """(DltSizeEstimator, lib) over tests/cpp/zstd_estimator.c -- a thread-safe C estimator on the system libzstd that
    counts its calls and its highest concurrency; None when gcc or libzstd is missing."""
    import os
    import subprocess

    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, "cpp", "zstd_estimator.c"), os.path.join(here, "cpp", "libzest.so")
    try:
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", src, "-o", so, "-ldl"])
        lib = C.CDLL(so)
    except (OSError, subprocess.CalledProcessError):
        return None
    lib.zest_init.restype = C.c_int
    if lib.zest_init() != 0:
        return None
    max_fn = C.cast(lib.zest_max_compressed_size, MAXFN)
    est_fn = C.cast(lib.zest_len_estimate if level is None else lib.zest_estimate, ESTFN)   # level None: size = len, in C
    est = DltSizeEstimator(C.c_void_p(level or 0), max_fn, est_fn)
    est._keep = (max_fn, est_fn, lib)
    return est, lib
