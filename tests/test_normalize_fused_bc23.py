"""BC2 / BC3 block normalisation fused into the forward transform (include/dxtlt_bc23_normalize.h,
dxtlt_transform_bc{2,3}_with_normalize_blocks[_device]): what can be shown without a device, and the case lists, data and
expectations that tests/test_normalize_fused_bc23_gpu.py runs on one.

Expected bytes are always oracle.transform(fmt, oracle.normalize_bcN_blocks(x, modes), settings), composed here (`expected`);
comparison is byte equality only.

1. The four symbols exist and carry the header's prototypes (fails where the calls do not exist).
2. Every invalid argument is answered with DXTLT_E_INVALID_ARGUMENT and a message, before any device work: alpha mode 4, colour
   mode 3, an alpha mode on BC2 (the BC2 calls have no such parameter: the launch layer's answer, which both formats' calls go
   through, is read through dxtlt_debug_check_normalization, and the Python wrapper takes none), len = 24, NULL pointers.
3. Data: classed_blocks of tests/test_normalize_alignment.py (structured_blocks rows of tests/test_normalize_bc23.py through a
   shuffle that is blind to the slot).  For every block count of the device tests and every mode pair: every class -- alpha kept /
   uniform / uniform and opaque, crossed with colour kept / solid -- at every i % 4 (counts from 64 blocks on: a class cannot sit
   at four slots in fewer blocks than there are classes x slots), normalised data != data, any two mode pairs give different
   expected bytes (so a kernel that ignores or mixes up the mode argument cannot pass; counts below 64 start at a block that all
   mode pairs treat differently), and the BC3 data holds neighbouring alpha endpoints (|a0 - a1| < 7) with several index values,
   some uniform by the oracle and some not: the walk in uniform_alpha_bc3.
4. Reach: through dxtlt_debug_plan_transform, the device tests' case list launches `tiled`, `halo[0]` and `halo[1]` of each of the
   8 + 16 kernel sets without a force bit, and the forced cases add the natural and the generic LDS form on zero shifts.  (The plan
   of a normalising call is the plain call's plan: the modes pick the kernel set, launch_transform in csrc/bcn_kernels.hip.)
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_alignment_sweep import (ALL_OFF, DEFAULT, SETTINGS, Case, aos_residue, build_cases, is_whole, lib, plan_of)  # noqa: F401
from test_normalize_alignment import class_table, classed_blocks, in_every_slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT_ID = {"bc2": 2, "bc3": 3}
FORMATS = ("bc2", "bc3")
E_INVALID_ARGUMENT = 2

# (alpha mode, colour mode): 2 pairs for BC2, 11 for BC3; (0, 0) is the plain transform
MODE_PAIRS = {"bc2": [(0, 1), (0, 2)], "bc3": [(a, c) for a in range(4) for c in range(3) if (a, c) != (0, 0)]}
SWEEP_MODES = {"bc2": (0, 2), "bc3": (3, 2)}
T = 256                                                       # blocks of the aligned tile: 256 lanes x 16 bytes / 16 bytes per block
PAIR_COUNTS = (1, T - 1, T, T + 1, 2 * T + 9, 3 * T)
PAIR_RESIDUES = (0, 1)
FORCED = (0x2, 0x20, 0x22)
FORCED_RESIDUES = (0, 64)
ROUND_TRIP_COUNT = 2 * T + 9
HOST_COUNTS = (4096 // 16 + 1, (1 << 20) // 16 + 1)           # 4 KiB + 16 bytes: mapped staging; 1 MiB + 16 bytes: one upload


def sweep_cases(fmt):
    """the BC2 / BC3 forward whole-buffer cases of test_alignment_sweep.build_cases"""
    return [c for c in build_cases(fmt) if not c.inverse and is_whole(c)]


def pair_cases(fmt):
    out = []
    for s in (DEFAULT[fmt], ALL_OFF):
        for n in PAIR_COUNTS:
            for p in PAIR_RESIDUES:
                out.append(Case(fmt, s, False, p, aos_residue(len(out)), n, 0, n))
    return out


def forced_cases(fmt, s):
    return [Case(fmt, s, False, p, aos_residue(i), 3 * T, 0, 3 * T) for i, p in enumerate(FORCED_RESIDUES)]


def round_trip_case(fmt, s):
    return Case(fmt, s, False, 1, 4, ROUND_TRIP_COUNT, 0, ROUND_TRIP_COUNT)


def device_counts(fmt):
    return sorted({c.num for c in sweep_cases(fmt)} | set(PAIR_COUNTS) | {ROUND_TRIP_COUNT})


# ------------------------------------------------------------------------------------------------------------
# data and expectations, computed once and read-only
# ------------------------------------------------------------------------------------------------------------
RUNS = 5
_POOL, _BLOCKS, _NORM, _WANT = {}, {}, {}, {}


def normalize(oracle, fmt, x, modes):
    return oracle.normalize_bc2_blocks(x, modes[1]) if fmt == "bc2" else oracle.normalize_bc3_blocks(x, modes[0], modes[1])


def told_apart_by_every_mode_pair(oracle, fmt, block):
    outs = {normalize(oracle, fmt, block, m).tobytes() for m in MODE_PAIRS[fmt]} | {block.tobytes()}
    return len(outs) == len(MODE_PAIRS[fmt]) + 1


def blocks_of(oracle, fmt, n):
    """the n blocks every test uses for that count.  Counts below 64 start at a block every mode pair treats differently."""
    if (fmt, n) not in _BLOCKS:
        if n in HOST_COUNTS:
            x = classed_blocks(fmt, oracle, n, 0xF23 + n)
        else:
            if fmt not in _POOL:
                _POOL[fmt] = classed_blocks(fmt, oracle, max(device_counts(fmt)) + 32 * (RUNS + 1), 0xF05ED23 + FMT_ID[fmt])
            first = 32 * (n % RUNS)
            if n < 64:
                first = next(i for i in range(first, first + 32)
                             if told_apart_by_every_mode_pair(oracle, fmt, _POOL[fmt][16 * i:16 * i + 16]))
            x = _POOL[fmt][16 * first:16 * (first + n)].copy()
        x.setflags(write=False)
        _BLOCKS[(fmt, n)] = x
    return _BLOCKS[(fmt, n)]


def normalized(oracle, fmt, n, modes):
    key = (fmt, n, modes)
    if key not in _NORM:
        y = blocks_of(oracle, fmt, n) if modes == (0, 0) else normalize(oracle, fmt, blocks_of(oracle, fmt, n), modes)
        y.setflags(write=False)
        _NORM[key] = y
    return _NORM[key]


def expected(oracle, fmt, s, n, modes):
    """oracle.transform_bcN(oracle.normalize_bcN_blocks(x, modes), settings)"""
    key = (fmt, s, n, modes)
    if key not in _WANT:
        v, sa, sc = s
        w = np.ascontiguousarray(oracle.transform(fmt, normalized(oracle, fmt, n, modes), v, bool(sc), bool(sa)))
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# ------------------------------------------------------------------------------------------------------------
# 1. symbols and prototypes
# ------------------------------------------------------------------------------------------------------------
PROTOTYPES = {
    "dxtlt_transform_bc2_with_normalize_blocks":
        "const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, uint8_t color_mode, uint8_t decorrelation_mode, "
        "bool split_colour_endpoints",
    "dxtlt_transform_bc2_with_normalize_blocks_device":
        "const void *d_input, void *d_output, size_t len, uint8_t color_mode, uint8_t decorrelation_mode, "
        "bool split_colour_endpoints, void *hip_stream",
    "dxtlt_transform_bc3_with_normalize_blocks":
        "const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, uint8_t alpha_mode, uint8_t color_mode, "
        "uint8_t decorrelation_mode, bool split_alpha_endpoints, bool split_colour_endpoints",
    "dxtlt_transform_bc3_with_normalize_blocks_device":
        "const void *d_input, void *d_output, size_t len, uint8_t alpha_mode, uint8_t color_mode, uint8_t decorrelation_mode, "
        "bool split_alpha_endpoints, bool split_colour_endpoints, void *hip_stream",
}
CTYPE = {"const uint8_t *": C.c_void_p, "uint8_t *": C.c_void_p, "const void *": C.c_void_p, "void *": C.c_void_p,
         "size_t": C.c_size_t, "uint8_t": C.c_uint8, "bool": C.c_bool}


def bound(pkg):
    """the four calls with the argument types the header states"""
    l = C.CDLL(pkg._lib.lib_path())
    for name, args in PROTOTYPES.items():
        f = getattr(l, name)
        f.restype = C.c_int32
        f.argtypes = [CTYPE[re.sub(r"\w+$", "", a.strip()).strip()] for a in args.split(",")]
    l.dxtlt_last_error.restype = C.c_char_p
    l.dxtlt_debug_check_normalization.restype = C.c_int32
    l.dxtlt_debug_check_normalization.argtypes = [C.c_int32, C.c_int32, C.c_uint8, C.c_uint8]
    return l


def test_the_four_symbols_exist_with_the_headers_prototypes(pkg):
    header = open(os.path.join(ROOT, "include", "dxtlt_bc23_normalize.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    l = C.CDLL(pkg._lib.lib_path())
    for name, args in PROTOTYPES.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name}: no prototype in include/dxtlt_bc23_normalize.h"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, name
        assert hasattr(l, name), f"{name}: not exported"


# ------------------------------------------------------------------------------------------------------------
# 2. invalid arguments
# ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_answered_before_any_device_work(pkg):
    from dxt_lossless_transform_amd import normalize as norm

    l = bound(pkg)
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data

    def refused(rc, what):
        text = l.dxtlt_last_error().decode()
        assert rc == E_INVALID_ARGUMENT and text.startswith("dxtlt: ") and len(text) > 10, (what, rc, text)
        return text

    bc2, bc2d = l.dxtlt_transform_bc2_with_normalize_blocks, l.dxtlt_transform_bc2_with_normalize_blocks_device
    bc3, bc3d = l.dxtlt_transform_bc3_with_normalize_blocks, l.dxtlt_transform_bc3_with_normalize_blocks_device
    assert "alpha_mode" in refused(bc3(p, p, 16, 4, 1, 1, True, True), "alpha mode 4")
    assert "alpha_mode" in refused(bc3d(p, p, 16, 4, 1, 1, True, True, None), "alpha mode 4, device")
    assert "color_mode" in refused(bc3(p, p, 16, 1, 3, 1, True, True), "colour mode 3")
    assert "color_mode" in refused(bc3d(p, p, 16, 1, 3, 1, True, True, None), "colour mode 3, device")
    assert "color_mode" in refused(bc2(p, p, 16, 3, 1, True), "colour mode 3, bc2")
    assert "color_mode" in refused(bc2d(p, p, 16, 3, 1, True, None), "colour mode 3, bc2, device")
    assert "decorrelation_mode" in refused(bc2(p, p, 16, 1, 4, True), "decorrelation mode 4")
    assert "decorrelation_mode" in refused(bc3d(p, p, 16, 1, 1, 4, True, True, None), "decorrelation mode 4")
    for what, rc in (("bc2", bc2(p, p, 24, 1, 1, True)), ("bc2 device", bc2d(p, p, 24, 1, 1, True, None)),
                     ("bc3", bc3(p, p, 24, 1, 1, 1, True, True)), ("bc3 device", bc3d(p, p, 24, 1, 1, 1, True, True, None))):
        assert "multiple of 16" in refused(rc, "len = 24, " + what)
    for a, b in ((None, p), (p, None), (None, None)):
        assert "NULL" in refused(bc2(a, b, 16, 1, 1, True), "NULL, bc2")
        assert "NULL" in refused(bc2d(a, b, 16, 1, 1, True, None), "NULL, bc2 device")
        assert "NULL" in refused(bc3(a, b, 16, 1, 1, 1, True, True), "NULL, bc3")
        assert "NULL" in refused(bc3d(a, b, 16, 1, 1, 1, True, True, None), "NULL, bc3 device")
    # zero blocks: nothing to do, no device needed, NULL allowed
    assert bc2(None, None, 0, 2, 1, True) == 0 and bc2d(None, None, 0, 2, 1, True, None) == 0
    assert bc3(None, None, 0, 3, 2, 1, True, True) == 0 and bc3d(None, None, 0, 3, 2, 1, True, True, None) == 0

    # the launch layer (both formats' calls end there): the table of the header
    check = l.dxtlt_debug_check_normalization
    for fmt in (1, 2, 3):
        assert all(check(fmt, 0, c, 0) == 0 for c in range(3))
        refused(check(fmt, 0, 4, 0), "colour mode 4")
        for c in range(3):
            refused(check(fmt, 1, max(c, 1), 0), "inverse")
    assert all(check(3, 0, c, a) == 0 for a in range(4) for c in range(3))
    refused(check(3, 0, 1, 4), "alpha mode 4")
    refused(check(3, 1, 0, 1), "inverse with an alpha mode")
    for a in (1, 2, 3):
        assert "alpha_mode" in refused(check(2, 0, 1, a), "an alpha mode on BC2")
        refused(check(2, 0, 0, a), "an alpha mode alone on BC2")
        refused(check(1, 0, 1, a), "an alpha mode on BC1")
    refused(check(2, 0, 3, 0), "BC1's transparent-only mode on BC2")
    assert check(1, 0, 3, 0) == 0                                     # (internal to BC1's auto transform)
    for fmt in (4, 5):
        refused(check(fmt, 0, 1, 0), "BC4 / BC5")
        refused(check(fmt, 0, 0, 1), "BC4 / BC5")
    # and the Python wrapper of the BC2 call has no alpha parameter to pass one through
    with pytest.raises(TypeError):
        norm.transform_bc2_with_normalize_blocks(buf[:16], buf[16:32], 1, alpha_mode=1)
    with pytest.raises(pkg.InvalidLength):
        norm.transform_bc3_with_normalize_blocks(buf[:24], buf[32:], 1, 1)
    with pytest.raises(pkg.DeviceError) as e:
        norm.transform_bc3_with_normalize_blocks(buf[:16], buf[16:32], 4, 1)
    assert e.value.code == E_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------------------
# 3. data
# ------------------------------------------------------------------------------------------------------------
CLASSES = {"bc2": ("colour kept", "colour solid"),
           "bc3": tuple(f"alpha {a}, colour {c}" for a in ("kept", "uniform", "uniform and opaque") for c in ("kept", "solid"))}


@pytest.mark.parametrize("fmt", FORMATS)
def test_data_holds_every_class_in_every_slot_and_tells_the_mode_pairs_apart(oracle, fmt):
    assert len(MODE_PAIRS["bc2"]) == 2 and len(MODE_PAIRS["bc3"]) == 11
    for n in device_counts(fmt) + list(HOST_COUNTS):
        x = blocks_of(oracle, fmt, n)
        b = x.reshape(-1, 16)
        if n >= 64:
            cls, count = class_table(fmt, oracle, b)
            assert count == len(CLASSES[fmt])
            for k, name in enumerate(CLASSES[fmt]):
                assert in_every_slot(cls == k), (fmt, n, name)
        outs = {}
        for m in MODE_PAIRS[fmt]:
            y = normalized(oracle, fmt, n, m)
            assert not np.array_equal(y, x), (fmt, n, m, "the normalised data is the data")
            if fmt == "bc2" or m[0] == 0:
                assert np.array_equal(y.reshape(-1, 16)[:, :8], b[:, :8]), (fmt, n, m, "alpha half touched")
            if m[1] == 0:
                assert np.array_equal(y.reshape(-1, 16)[:, 8:], b[:, 8:]), (fmt, n, m, "colour half touched")
            outs[m] = y.tobytes()
        assert len(set(outs.values())) == len(MODE_PAIRS[fmt]), (fmt, n, "two mode pairs normalise alike")
        # the expectations themselves (the transform is a bijection, so this follows; stated on the default and the all-off settings)
        if n in PAIR_COUNTS:
            for s in (DEFAULT[fmt], ALL_OFF):
                wants = {expected(oracle, fmt, s, n, m).tobytes() for m in MODE_PAIRS[fmt] + [(0, 0)]}
                assert len(wants) == len(MODE_PAIRS[fmt]) + 1, (fmt, s, n)


def test_bc3_data_walks_neighbouring_alpha_endpoints(oracle):
    """|a0 - a1| < 7 with several index values: uniform_alpha_bc3 (csrc/bc23_normalize.h) cannot decide from the endpoints and walks
    the sixteen indices.  Some such blocks are uniform by the oracle -- table entries coincide -- and some are not."""
    for n in device_counts("bc3") + list(HOST_COUNTS):
        if n < 64:
            continue
        b = blocks_of(oracle, "bc3", n).reshape(-1, 16)
        near = np.abs(b[:, 0].astype(np.int64) - b[:, 1].astype(np.int64)) < 7
        bits = sum(b[:, 2 + k].astype(np.uint64) << np.uint64(8 * k) for k in range(6))
        first = bits & np.uint64(7)
        several = bits != first * np.uint64(0x249249249249)
        uniform = (normalized(oracle, "bc3", n, (1, 0)).reshape(-1, 16)[:, :8] != b[:, :8]).any(axis=1)
        already = (b[:, 1:8] == 0).all(axis=1)                         # (alpha, 0, indices 0): uniform, and nothing to rewrite
        walk = near & several
        assert (walk & uniform).sum() >= 2 and (walk & ~uniform & ~already).sum() >= 2, (n, int((walk & uniform).sum()), int(walk.sum()))


# ------------------------------------------------------------------------------------------------------------
# 4. reach
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_case_list_reaches_every_member_of_every_kernel_set(pkg, lib, fmt):
    assert len(SETTINGS[fmt]) == (8 if fmt == "bc2" else 16)
    pkg.set_tuning(0, 0)
    members = {s: set() for s in SETTINGS[fmt]}
    for c in sweep_cases(fmt) + pair_cases(fmt):
        for l in plan_of(lib, c):
            assert l.kind in (0, 1) and l.threads == 256
            members[c.settings].add("tiled" if l.kind == 0 else f"halo[{l.natural}]")
    assert all(m == {"tiled", "halo[0]", "halo[1]"} for m in members.values()), members
    # every mode pair meets all three members too: on the default and the all-off settings, at residues 0 (3T: aligned) and 1
    for s in (DEFAULT[fmt], ALL_OFF):
        seen = {("tiled" if l.kind == 0 else f"halo[{l.natural}]") for c in pair_cases(fmt) if c.settings == s for l in plan_of(lib, c)}
        assert seen >= {"tiled", "halo[0]"}, (s, seen)
    # one round-trip case per kernel set, in the halo tiles with full tiles and a tail
    for s in SETTINGS[fmt]:
        (l,) = plan_of(lib, round_trip_case(fmt, s))
        assert l.kind == 1 and l.full_tiles == 2 and l.workgroups == 3
    try:
        for s in SETTINGS[fmt]:
            seen = set()
            for f in FORCED:
                pkg.set_tuning(0, f)
                for c in forced_cases(fmt, s):
                    launches = plan_of(lib, c)
                    # (residue 64: bases off their 128-byte lines, halo tiles by themselves, with zero shifts modulo 64)
                    assert [l.kind for l in launches] == ([1] if f & 2 or c.p % 128 else [0]), (s, f, c)
                    for l in launches:
                        if l.kind:
                            assert not (f & 0x20 and l.natural) and not any(l.shift) and l.workgroups == l.full_tiles == 3
                            seen.add((f, l.natural))
            # bit 2 moves the aligned buffers into the halo tiles: the natural and, with 0x20, the generic LDS form on zero shifts
            assert seen == {(0x2, 1), (0x20, 0), (0x22, 0)}, (s, seen)
    finally:
        pkg.set_tuning(0, 0)
    assert all(c.num == 3 * T for s in SETTINGS[fmt] for c in forced_cases(fmt, s))
    assert {c.p for c in forced_cases(fmt, DEFAULT[fmt])} == set(FORCED_RESIDUES)
