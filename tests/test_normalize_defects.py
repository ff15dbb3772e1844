"""What the 25 block-normalisation entry points (include/dxtlt_bc1_normalize.h, include/dxtlt_bc23_normalize.h) answer to
defective arguments, before any device work: the returned status and one distinguishing word of dxtlt_last_error(), as literals.

Per entry point: a length that is no whole number of blocks, each mode one past its range, NULL in every pointer position (the
output pointer array itself and each single element of it included), zero length / zero blocks with NULL pointers (OK), pairs of
defects in one call (they pin the order of the checks), and the shortcuts that do no device work (mode None on host pointers is a
copy, or nothing in place; *out_any_normalized is cleared before the length-0 return).

Asymmetries that are part of the table: the BC1 fused calls answer a bad length with INVALID_LENGTH, the BC2 / BC3 fused calls
with INVALID_ARGUMENT; the BC1 fused host call checks the colour mode, then the length, then the decorrelation mode, then NULL,
while its _device twin checks the length first; dxtlt_bc2_normalize_split_blocks_in_place ignores its alpha_ptr;
d_any_normalized may be NULL."""
import ctypes as C

import numpy as np
import pytest

OK, E_LENGTH, E_ARGUMENT = 0, 1, 2

vp, sz, u8, b = C.c_void_p, C.c_size_t, C.c_uint8, C.c_bool
pp = C.POINTER(vp)

MAX_FN = C.CFUNCTYPE(C.c_uint32, vp, sz, C.POINTER(sz))
EST_FN = C.CFUNCTYPE(C.c_uint32, vp, vp, sz, vp, sz, C.POINTER(sz))


class Estimator(C.Structure):
    _fields_ = [("Context", vp), ("MaxCompressedSize", MAX_FN), ("EstimateCompressedSize", EST_FN)]


ARGTYPES = {
    "dxtlt_bc1_normalize_blocks": [vp, vp, sz, u8],
    "dxtlt_bc1_normalize_blocks_device": [vp, vp, sz, u8, vp],
    "dxtlt_bc1_normalize_split_blocks_in_place": [vp, vp, sz, u8],
    "dxtlt_bc1_normalize_split_blocks_in_place_device": [vp, vp, sz, u8, vp],
    "dxtlt_bc1_normalize_blocks_all_modes": [vp, pp, sz, C.POINTER(b)],
    "dxtlt_bc1_normalize_blocks_all_modes_device": [vp, pp, sz, vp, vp],
    "dxtlt_transform_bc1_with_normalize_blocks": [vp, vp, vp, sz, u8, u8, b],
    "dxtlt_transform_bc1_with_normalize_blocks_device": [vp, vp, sz, u8, u8, b, vp],
    "dxtlt_transform_bc1_auto_with_normalization": [vp, vp, sz, C.POINTER(Estimator), b, C.POINTER(u8), C.POINTER(u8), C.POINTER(b),
                                                    C.POINTER(C.c_uint32)],
    "dxtlt_bc2_normalize_blocks": [vp, vp, sz, u8],
    "dxtlt_bc2_normalize_blocks_device": [vp, vp, sz, u8, vp],
    "dxtlt_bc3_normalize_blocks": [vp, vp, sz, u8, u8],
    "dxtlt_bc3_normalize_blocks_device": [vp, vp, sz, u8, u8, vp],
    "dxtlt_bc2_normalize_split_blocks_in_place": [vp, vp, vp, sz, u8],
    "dxtlt_bc2_normalize_split_blocks_in_place_device": [vp, vp, sz, u8, vp],
    "dxtlt_bc3_normalize_split_blocks_in_place": [vp, vp, vp, vp, sz, u8, u8],
    "dxtlt_bc3_normalize_split_blocks_in_place_device": [vp, vp, vp, vp, sz, u8, u8, vp],
    "dxtlt_bc2_normalize_blocks_all_modes": [vp, pp, sz],
    "dxtlt_bc2_normalize_blocks_all_modes_device": [vp, pp, sz, vp],
    "dxtlt_bc3_normalize_blocks_all_modes": [vp, pp, sz],
    "dxtlt_bc3_normalize_blocks_all_modes_device": [vp, pp, sz, vp],
    "dxtlt_transform_bc2_with_normalize_blocks": [vp, vp, sz, u8, u8, b],
    "dxtlt_transform_bc2_with_normalize_blocks_device": [vp, vp, sz, u8, u8, b, vp],
    "dxtlt_transform_bc3_with_normalize_blocks": [vp, vp, sz, u8, u8, u8, b, b],
    "dxtlt_transform_bc3_with_normalize_blocks_device": [vp, vp, sz, u8, u8, u8, b, b, vp],
}


def test_the_table_names_all_25_entry_points():
    assert len(ARGTYPES) == 25


class Lib:
    """the library with the headers' argument types; calls return (status, error text)"""

    def __init__(self, pkg):
        self.l = C.CDLL(pkg._lib.lib_path())
        for name, args in ARGTYPES.items():
            f = getattr(self.l, name)
            f.argtypes, f.restype = args, C.c_int32
        self.l.dxtlt_last_error.restype = C.c_char_p

    def __getattr__(self, name):
        f = getattr(self.l, "dxtlt_" + name)
        return lambda *args: (f(*args), self.l.dxtlt_last_error().decode())


@pytest.fixture(scope="module")
def lib(pkg):
    return Lib(pkg)


def refused(answer, code, word):
    rc, text = answer
    assert rc == code and text.startswith("dxtlt: ") and word in text, (answer, code, word)


def ok(answer):
    assert answer[0] == OK, answer


BUF = np.arange(64, dtype=np.uint8)
P = BUF.ctypes.data


def ptr_array(count, null_at=None):
    return (vp * count)(*[None if k == null_at else P for k in range(count)])


# ------------------------------------------------------------------------------------------------------------
# AoS blocks: dxtlt_bcN_normalize_blocks[_device]
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", (False, True))
def test_bc1_blocks(lib, device):
    f = (lambda i, o, n, c: lib.bc1_normalize_blocks_device(i, o, n, c, None)) if device else lib.bc1_normalize_blocks
    refused(f(P, P, 12, 1), E_LENGTH, "multiple of 8")
    refused(f(P, P, 16, 3), E_ARGUMENT, "color_mode")
    for i, o in ((None, P), (P, None), (None, None)):
        refused(f(i, o, 16, 1), E_ARGUMENT, "NULL")
    ok(f(None, None, 0, 2))
    # order: length, colour mode, NULL; the mode is checked before the length-0 return
    refused(f(None, None, 12, 3), E_LENGTH, "multiple of 8")
    refused(f(None, None, 16, 3), E_ARGUMENT, "color_mode")
    refused(f(None, None, 0, 3), E_ARGUMENT, "color_mode")


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("fmt", (2, 3))
def test_bc23_blocks(lib, fmt, device):
    name = f"bc{fmt}_normalize_blocks" + ("_device" if device else "")
    tail = (None,) if device else ()

    def f(i, o, n, a, c):
        return getattr(lib, name)(i, o, n, *((a, c) if fmt == 3 else (c,)), *tail)

    refused(f(P, P, 24, 0, 1), E_LENGTH, "multiple of 16")
    refused(f(P, P, 16, 0, 3), E_ARGUMENT, "color_mode")
    if fmt == 3:
        refused(f(P, P, 16, 4, 1), E_ARGUMENT, "alpha_mode")
        refused(f(P, P, 16, 4, 3), E_ARGUMENT, "color_mode")           # colour before alpha
        refused(f(None, None, 16, 4, 1), E_ARGUMENT, "alpha_mode")     # modes before NULL
        refused(f(None, None, 24, 4, 1), E_LENGTH, "multiple of 16")   # length before modes
        refused(f(None, None, 0, 4, 0), E_ARGUMENT, "alpha_mode")      # modes before the length-0 return
    for i, o in ((None, P), (P, None), (None, None)):
        refused(f(i, o, 16, 1 if fmt == 3 else 0, 1), E_ARGUMENT, "NULL")
    ok(f(None, None, 0, 3 if fmt == 3 else 0, 2))
    refused(f(None, None, 24, 0, 3), E_LENGTH, "multiple of 16")
    refused(f(None, None, 16, 0, 3), E_ARGUMENT, "color_mode")
    refused(f(None, None, 0, 0, 3), E_ARGUMENT, "color_mode")


def test_mode_none_on_host_pointers_is_a_copy_or_nothing_in_place(lib):
    src = np.arange(32, dtype=np.uint8)
    for call in (lambda i, o: lib.bc1_normalize_blocks(i, o, 32, 0), lambda i, o: lib.bc2_normalize_blocks(i, o, 32, 0),
                 lambda i, o: lib.bc3_normalize_blocks(i, o, 32, 0, 0)):
        dst = np.full(40, 0xEE, dtype=np.uint8)
        ok(call(src.ctypes.data, dst.ctypes.data))
        assert np.array_equal(dst[:32], src) and (dst[32:] == 0xEE).all()
        same = src.copy()
        ok(call(same.ctypes.data, same.ctypes.data))
        assert np.array_equal(same, src)
        # but NULL is refused first
        refused(call(None, dst.ctypes.data), E_ARGUMENT, "NULL")


# ------------------------------------------------------------------------------------------------------------
# split arrays in place
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (1, 2))
def test_two_array_split_device(lib, fmt):
    f = getattr(lib, f"bc{fmt}_normalize_split_blocks_in_place_device")
    refused(f(P, P, 2, 3, None), E_ARGUMENT, "color_mode")
    for c, x in ((None, P), (P, None), (None, None)):
        refused(f(c, x, 2, 1, None), E_ARGUMENT, "NULL")
        refused(f(c, x, 2, 0, None), E_ARGUMENT, "NULL")               # the device form has no mode-None return before NULL
    ok(f(None, None, 0, 2, None))
    refused(f(None, None, 2, 3, None), E_ARGUMENT, "color_mode")       # mode before NULL
    refused(f(None, None, 0, 3, None), E_ARGUMENT, "color_mode")


def test_bc1_split_host(lib):
    f = lib.bc1_normalize_split_blocks_in_place
    refused(f(P, P, 2, 3), E_ARGUMENT, "color_mode")
    for c, x in ((None, P), (P, None), (None, None)):
        refused(f(c, x, 2, 1), E_ARGUMENT, "NULL")
        ok(f(c, x, 2, 0))                                              # mode None returns before the NULL check
    ok(f(None, None, 0, 2))
    refused(f(None, None, 2, 3), E_ARGUMENT, "color_mode")
    refused(f(None, None, 0, 3), E_ARGUMENT, "color_mode")
    before = BUF.copy()
    ok(f(P, P + 32, 4, 0))
    assert np.array_equal(BUF, before)


def test_bc2_split_host_ignores_its_alpha_pointer(lib):
    f = lib.bc2_normalize_split_blocks_in_place
    for alpha in (None, P):
        refused(f(alpha, P, P, 2, 3), E_ARGUMENT, "color_mode")
        for c, x in ((None, P), (P, None), (None, None)):
            refused(f(alpha, c, x, 2, 1), E_ARGUMENT, "NULL")
            ok(f(alpha, c, x, 2, 0))
        ok(f(alpha, None, None, 0, 2))
        refused(f(alpha, None, None, 2, 3), E_ARGUMENT, "color_mode")
        refused(f(alpha, None, None, 0, 3), E_ARGUMENT, "color_mode")
    # a NULL alpha array with everything else in order is no defect: the call goes on to the device (OK with one, NO_DEVICE / DEVICE without)
    c, x = np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.uint8)
    rc, text = f(None, c.ctypes.data, x.ctypes.data, 2, 1)
    assert rc in (0, 3, 4), (rc, text)


@pytest.mark.parametrize("device", (False, True))
def test_bc3_split(lib, device):
    name = "bc3_normalize_split_blocks_in_place" + ("_device" if device else "")
    tail = (None,) if device else ()

    def f(ptrs, n, a, c):
        return getattr(lib, name)(*ptrs, n, a, c, *tail)

    all4 = (P, P, P, P)
    refused(f(all4, 2, 1, 3), E_ARGUMENT, "color_mode")
    refused(f(all4, 2, 4, 1), E_ARGUMENT, "alpha_mode")
    refused(f(all4, 2, 4, 3), E_ARGUMENT, "color_mode")                # colour before alpha
    for k in range(4):
        ptrs = tuple(None if j == k else P for j in range(4))
        refused(f(ptrs, 2, 1, 1), E_ARGUMENT, "NULL")
        refused(f(ptrs, 2, 0, 1), E_ARGUMENT, "NULL")
        refused(f(ptrs, 2, 1, 0), E_ARGUMENT, "NULL")
        if device:
            refused(f(ptrs, 2, 0, 0), E_ARGUMENT, "NULL")
        else:
            ok(f(ptrs, 2, 0, 0))                                       # both modes None: returns before the NULL check
    none4 = (None,) * 4
    ok(f(none4, 0, 3, 2))
    refused(f(none4, 2, 4, 1), E_ARGUMENT, "alpha_mode")               # modes before NULL
    refused(f(none4, 0, 4, 1), E_ARGUMENT, "alpha_mode")               # and before the zero-blocks return
    refused(f(none4, 0, 1, 3), E_ARGUMENT, "color_mode")


# ------------------------------------------------------------------------------------------------------------
# all modes
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("fmt,count", ((1, 3), (2, 3), (3, 12)))
def test_all_modes(lib, fmt, count, device):
    name = f"bc{fmt}_normalize_blocks_all_modes" + ("_device" if device else "")
    block = 8 if fmt == 1 else 16
    flag = b(True)
    if fmt == 1:
        tail = (None, None) if device else (C.byref(flag),)           # d_any_normalized may be NULL
    else:
        tail = (None,) if device else ()

    def f(i, outs, n):
        return getattr(lib, name)(i, outs, n, *tail)

    refused(f(P, ptr_array(count), block + block // 2), E_LENGTH, f"multiple of {block}")
    refused(f(P, None, block), E_ARGUMENT, "NULL")
    refused(f(None, None, 0), E_ARGUMENT, "NULL")                      # the array itself is needed at length 0 too
    refused(f(None, None, block + 4), E_LENGTH, f"multiple of {block}")   # length before the array
    refused(f(None, ptr_array(count), block), E_ARGUMENT, "NULL")
    for k in range(count):
        refused(f(P, ptr_array(count, null_at=k), block), E_ARGUMENT, "NULL")
    ok(f(None, ptr_array(count, null_at=0), 0))
    ok(f(None, (vp * count)(), 0))


def test_bc1_all_modes_clears_its_flag_before_the_length_0_return(lib):
    f = lib.bc1_normalize_blocks_all_modes
    flag = b(True)
    refused(f(P, ptr_array(3), 12, C.byref(flag)), E_LENGTH, "multiple of 8")
    assert flag.value is True                                          # not yet
    refused(f(P, None, 8, C.byref(flag)), E_ARGUMENT, "NULL")
    assert flag.value is True
    ok(f(None, ptr_array(3), 0, C.byref(flag)))
    assert flag.value is False
    flag = b(True)
    refused(f(None, ptr_array(3), 8, C.byref(flag)), E_ARGUMENT, "NULL")
    assert flag.value is False                                         # cleared before the NULL check
    ok(f(None, ptr_array(3), 0, None))                                 # and optional


# ------------------------------------------------------------------------------------------------------------
# fused normalise + transform
# ------------------------------------------------------------------------------------------------------------
def test_bc1_fused_host(lib):
    def f(i, o, n, c, d, work=None):
        return lib.transform_bc1_with_normalize_blocks(i, o, work, n, c, d, True)

    refused(f(P, P, 16, 3, 1), E_ARGUMENT, "color_mode")
    refused(f(P, P, 12, 1, 1), E_LENGTH, "multiple of")
    refused(f(P, P, 16, 1, 4), E_ARGUMENT, "decorrelation_mode")
    for i, o in ((None, P), (P, None), (None, None)):
        refused(f(i, o, 16, 1, 1), E_ARGUMENT, "NULL")
        refused(f(i, o, 16, 1, 1, work=P), E_ARGUMENT, "NULL")
    ok(f(None, None, 0, 2, 3))
    # order: colour mode, length, decorrelation mode, NULL
    refused(f(None, None, 12, 3, 4), E_ARGUMENT, "color_mode")
    refused(f(None, None, 12, 1, 4), E_LENGTH, "multiple of")
    refused(f(None, None, 16, 1, 4), E_ARGUMENT, "decorrelation_mode")
    refused(f(None, None, 0, 1, 4), E_ARGUMENT, "decorrelation_mode")


def test_bc1_fused_device(lib):
    def f(i, o, n, c, d):
        return lib.transform_bc1_with_normalize_blocks_device(i, o, n, c, d, True, None)

    refused(f(P, P, 16, 3, 1), E_ARGUMENT, "color_mode")
    refused(f(P, P, 12, 1, 1), E_LENGTH, "multiple of 8")
    refused(f(P, P, 16, 1, 4), E_ARGUMENT, "decorrelation_mode")
    for i, o in ((None, P), (P, None), (None, None)):
        refused(f(i, o, 16, 1, 1), E_ARGUMENT, "NULL")
    ok(f(None, None, 0, 2, 3))
    # order: length, colour mode, decorrelation mode, NULL
    refused(f(None, None, 12, 3, 4), E_LENGTH, "multiple of 8")
    refused(f(None, None, 16, 3, 4), E_ARGUMENT, "color_mode")
    refused(f(None, None, 16, 1, 4), E_ARGUMENT, "decorrelation_mode")
    refused(f(None, None, 0, 1, 4), E_ARGUMENT, "decorrelation_mode")


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("fmt", (2, 3))
def test_bc23_fused(lib, fmt, device):
    name = f"transform_bc{fmt}_with_normalize_blocks" + ("_device" if device else "")
    tail = (None,) if device else ()

    def f(i, o, n, a, c, d):
        modes = (a, c, d, True, True) if fmt == 3 else (c, d, True)
        return getattr(lib, name)(i, o, n, *modes, *tail)

    refused(f(P, P, 24, 0, 1, 1), E_ARGUMENT, "multiple of 16")        # INVALID_ARGUMENT, where BC1 answers INVALID_LENGTH
    refused(f(P, P, 16, 0, 3, 1), E_ARGUMENT, "color_mode")
    refused(f(P, P, 16, 0, 1, 4), E_ARGUMENT, "decorrelation_mode")
    if fmt == 3:
        refused(f(P, P, 16, 4, 1, 1), E_ARGUMENT, "alpha_mode")
        refused(f(P, P, 16, 4, 3, 1), E_ARGUMENT, "color_mode")        # colour before alpha
        refused(f(None, None, 24, 4, 1, 4), E_ARGUMENT, "alpha_mode")  # alpha before decorrelation
    for i, o in ((None, P), (P, None), (None, None)):
        refused(f(i, o, 16, 0, 1, 1), E_ARGUMENT, "NULL")
    ok(f(None, None, 0, 3 if fmt == 3 else 0, 2, 3))
    # order: normalisation modes, decorrelation mode, length, NULL
    refused(f(None, None, 24, 0, 3, 4), E_ARGUMENT, "color_mode")
    refused(f(None, None, 24, 0, 1, 4), E_ARGUMENT, "decorrelation_mode")
    refused(f(None, None, 24, 0, 1, 1), E_ARGUMENT, "multiple of 16")
    refused(f(None, None, 0, 0, 1, 4), E_ARGUMENT, "decorrelation_mode")


# ------------------------------------------------------------------------------------------------------------
# the BC1 auto transform with normalisation
# ------------------------------------------------------------------------------------------------------------
def test_bc1_auto_with_normalization(lib):
    calls = []

    def max_size(_ctx, n, out):
        calls.append(("max", n))
        out[0] = 0
        return 0

    def estimate(_ctx, _in, n, _scratch, _cap, out):
        calls.append(("estimate", n))
        out[0] = n
        return 0

    est = Estimator(None, MAX_FN(max_size), EST_FN(estimate))
    err = C.c_uint32(77)

    def f(i, o, n, e, err_ptr=None):
        return lib.transform_bc1_auto_with_normalization(i, o, n, e, False, None, None, None, err_ptr)

    refused(f(P, P, 12, C.byref(est), C.byref(err)), E_LENGTH, "multiple of 8")
    assert err.value == 0                                              # cleared first of all
    refused(f(P, P, 16, None), E_ARGUMENT, "estimator")
    no_max = Estimator(None, MAX_FN(), EST_FN(estimate))
    no_estimate = Estimator(None, MAX_FN(max_size), EST_FN())
    refused(f(P, P, 16, C.byref(no_max)), E_ARGUMENT, "estimator")
    refused(f(P, P, 16, C.byref(no_estimate)), E_ARGUMENT, "estimator")
    for i, o in ((None, P), (P, None), (None, None)):
        refused(f(i, o, 16, C.byref(est)), E_ARGUMENT, "NULL buffer")
    # order: length, estimator, buffers
    refused(f(None, None, 12, None), E_LENGTH, "multiple of 8")
    refused(f(None, None, 16, None), E_ARGUMENT, "estimator")
    refused(f(None, None, 0, None), E_ARGUMENT, "estimator")
    assert calls == []                                                 # no callback before the arguments are in order


def test_bc1_auto_with_normalization_propagates_the_size_query_before_any_device_work(lib):
    def max_size(_ctx, _n, _out):
        return 41

    def estimate(_ctx, _in, _n, _scratch, _cap, _out):
        return 0

    est = Estimator(None, MAX_FN(max_size), EST_FN(estimate))
    err = C.c_uint32(0)
    rc, text = lib.transform_bc1_auto_with_normalization(P, P, 16, C.byref(est), False, None, None, None, C.byref(err))
    assert rc == 5 and "estimator" in text and err.value == 41
