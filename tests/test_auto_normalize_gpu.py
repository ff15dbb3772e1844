"""The auto transform with block normalisation on the device (include/dxtlt_auto_normalize.h), held to the CPU statements of
tests/auto_normalize_ref.py: the candidate kernel's arena byte for byte, the whole device call -- choice, output bytes, totals and
what it waited for and launched --, the routes without the arena, the host calls (BC2's callback route under a scripted estimator
included), a capturing stream and the Python wrappers.
Every comparison is exact equality; every buffer the library writes lies between 256 guard bytes."""
import ctypes as C

import numpy as np
import pytest

import auto_normalize_ref as A
import cabi

pytestmark = pytest.mark.gpu

DEPTHS = [(1, False), (1, True), (2, False), (2, True)]
COUNTS = (1, 2, 3, 511, 512, 513, 1025)          # 512 BC1 blocks: one full workgroup; the odd BC1 counts: the last-block kernel
CALL_BLOCKS = (1, 2, 4097, 20001)                # 20 001: three estimator windows per section, the last one short
GUARD_FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return A.load(pkg)


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """n device bytes at `off` bytes past a 256-byte boundary, 256 guard bytes and more in front and behind"""

    def __init__(self, dev, n, off=0, data=None, fill=GUARD_FILL):
        import torch

        self.n, self.at, self.fill = n, A.GUARD + off, fill
        self.base = torch.full((self.at + n + A.GUARD,), fill, dtype=torch.uint8, device=dev)
        assert self.base.data_ptr() % 256 == 0
        if data is not None:
            self.base[self.at:self.at + n].copy_(torch.from_numpy(np.array(data)).to(dev))
        self.ptr = self.base.data_ptr() + self.at

    def bytes(self):
        """the payload, after checking the guards (synchronises)"""
        host = self.base.cpu().numpy()
        assert (host[:self.at] == self.fill).all() and (host[self.at + self.n:] == self.fill).all(), "guard bytes were written"
        return host[self.at:self.at + self.n]


def device_call(lib, dev, fmt, use_all, x, in_off=0):
    """(status, (norm, mode, split), output bytes, totals, last) of one device call; the input is checked to be unchanged"""
    import torch

    src, dst = Guarded(dev, x.size, in_off, x), Guarded(dev, x.size)
    norm, mode, split = C.c_uint8(0xEE), C.c_uint8(0xEE), C.c_bool(False)
    f = getattr(lib, f"dxtlt_transform_bc{fmt}_auto_with_normalization_device")
    rc = f(src.ptr, dst.ptr, x.size, use_all, stream(), C.byref(norm), C.byref(mode), C.byref(split))
    assert rc == A.OK, lib.dxtlt_last_error()
    last, totals = A.last(lib), A.last_totals(lib)
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), x), "the input was written"
    return (norm.value, mode.value, int(split.value)), dst.bytes(), totals, last


def candidate_launches(fmt, n):
    return (1 if n // 2 else 0) + n % 2 if fmt == 1 else 1


def check_against_statement(fmt, use_all, n, got, want, route="arena"):
    choice, out, totals, last = got
    want_choice, want_out, want_totals, any_normalized = want
    assert choice == want_choice, (n, choice, want_choice)
    assert totals == want_totals, n
    assert np.array_equal(out, want_out), (n, int(np.nonzero(out != want_out)[0][0]))
    if not any_normalized:
        assert last == [2, 0, 0, 0], (n, last)
    elif route == "arena":
        assert last == [2, candidate_launches(fmt, n), 2 if use_all else 1, 1], (n, last)
    else:                                                       # one fused transform and one estimate per candidate
        assert last == [2, len(want_totals), len(want_totals), 1], (n, last)


# ---- the candidate kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,use_all", DEPTHS)
def test_candidate_kernel_bytes(lib, dev, oracle, fmt, use_all):
    """every section == the colour section of transform(normalized[norm], variant, split) from the CPU; the guards around the arena and
    the input are untouched"""
    import torch

    hook = lib.dxtlt_debug_auto_normalization_candidates_into_device
    runs = []
    for n in COUNTS:
        x, want = A.arena_case(fmt, use_all, n)
        src, arena = Guarded(dev, x.size, 0, x), Guarded(dev, want.size, 0, None, A.FILL)
        assert hook(fmt, use_all, src.ptr, x.size, arena.ptr, want.size, stream()) == A.OK, (n, lib.dxtlt_last_error())
        runs.append((n, x, want, src, arena))
    torch.cuda.synchronize()
    for n, x, want, src, arena in runs:
        got = arena.bytes()
        for norm, v, sc, off, length in A.sections(use_all, n):
            bad = np.nonzero(got[off:off + length] != want[off:off + length])[0]
            assert bad.size == 0, f"{n} blocks, section (norm {norm}, variant {v}, split {sc}): {bad.size} bytes differ, first at {int(bad[0])}"
        assert np.array_equal(src.bytes(), x), "the input was written"


def test_candidate_hook_refusals_write_nothing(lib, dev, oracle):
    import torch

    x, want = A.arena_case(2, False, 513)
    src, arena = Guarded(dev, x.size, 0, x), Guarded(dev, want.size, 0, None, A.FILL)
    hook, s = lib.dxtlt_debug_auto_normalization_candidates_into_device, stream()
    for fmt in (0, 3, 4, 5, -1):
        assert hook(fmt, False, src.ptr, x.size, arena.ptr, want.size, s) == A.E_ARGUMENT, fmt
    assert hook(2, False, src.ptr, x.size - 8, arena.ptr, want.size, s) == A.E_ARGUMENT
    for off in (1, 4, 8):
        assert hook(2, False, src.ptr + off, x.size - 16, arena.ptr, want.size, s) == A.E_ARGUMENT, off
        assert hook(2, False, src.ptr, x.size - 16, arena.ptr + off, want.size - off, s) == A.E_ARGUMENT, off
    assert hook(2, False, src.ptr, x.size, arena.ptr, want.size - 1, s) == A.E_ARGUMENT and b"arena" in lib.dxtlt_last_error()
    assert hook(2, True, src.ptr, x.size, arena.ptr, want.size, s) == A.E_ARGUMENT            # all modes: twice the sections
    assert hook(2, False, None, x.size, arena.ptr, want.size, s) == A.E_ARGUMENT
    assert hook(2, False, src.ptr, x.size, None, want.size, s) == A.E_ARGUMENT
    torch.cuda.synchronize()
    assert (arena.bytes() == A.FILL).all()
    assert hook(2, False, src.ptr, x.size, arena.ptr, want.size, s) == A.OK                     # and the hook still works
    torch.cuda.synchronize()
    assert np.array_equal(arena.bytes(), want)


# ---- the whole device call -----------------------------------------------------------------------------------------------------------
CALL_CASES = [(fmt, use_all, kind) for fmt, use_all in DEPTHS for kind in A.KINDS if fmt == 1 or kind != "transparents"]


@pytest.mark.parametrize("fmt,use_all,kind", CALL_CASES)
def test_device_call_equals_the_statement(lib, dev, oracle, fmt, use_all, kind):
    for n in CALL_BLOCKS:
        x, want = A.case(fmt, kind, n, use_all)
        got = device_call(lib, dev, fmt, use_all, x)
        check_against_statement(fmt, use_all, n, got, want)
        assert A.last_estimation(lib) == (0, 0)
        if kind == "none":
            assert not want[3] and got[3][3] == 0
            plain = getattr(lib, f"dxtlt_transform_bc{fmt}_auto_device")
            src, dst = Guarded(dev, x.size, 0, x), Guarded(dev, x.size)
            mode, split = C.c_uint8(0xEE), C.c_bool(False)
            assert plain(src.ptr, dst.ptr, x.size, use_all, stream(), C.byref(mode), C.byref(split)) == A.OK
            assert A.last_totals(lib) == got[2]
            assert (A.NONE, mode.value, int(split.value)) == got[0] and np.array_equal(dst.bytes(), got[1])
        elif n > 2:
            assert want[3] and got[3][3] == 1


def test_every_mode_wins_on_the_device(lib, dev, oracle):
    """the data on which the CPU statement picks Color0Only, ReplicateColor and None: the device picks them too"""
    won = set()
    for fmt, kind in ((1, "cycle"), (1, "solids"), (2, "solids"), (1, "none")):
        x, want = A.case(fmt, kind, 4097, False)
        got = device_call(lib, dev, fmt, False, x)
        check_against_statement(fmt, False, 4097, got, want)
        won.add(got[0][0])
    assert won == {A.NONE, A.COLOR0_ONLY, A.REPLICATE_COLOR}


def test_empty_input(lib, dev):
    norm, mode, split = C.c_uint8(0xEE), C.c_uint8(0xEE), C.c_bool(True)
    for fmt, use_all in DEPTHS:
        f = getattr(lib, f"dxtlt_transform_bc{fmt}_auto_with_normalization_device")
        assert f(None, None, 0, use_all, stream(), C.byref(norm), C.byref(mode), C.byref(split)) == A.OK
        plain_mode, plain_split = C.c_uint8(0xEE), C.c_bool(True)
        assert getattr(lib, f"dxtlt_transform_bc{fmt}_auto_device")(None, None, 0, use_all, stream(), C.byref(plain_mode), C.byref(plain_split)) == A.OK
        assert (norm.value, mode.value, split.value) == (A.NONE, plain_mode.value, plain_split.value)


# ---- the other routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,use_all", DEPTHS)
def test_unaligned_input_and_no_arena_make_the_same_choice(lib, dev, oracle, fmt, use_all):
    for n, kind in ((4097, "cycle"), (513, "solids"), (513, "none")):
        x, want = A.case(fmt, kind, n, use_all)
        for off in (1, 4, 8):
            got = device_call(lib, dev, fmt, use_all, x, in_off=off)
            check_against_statement(fmt, use_all, n, got, want, route="one by one")
        lib.dxtlt_debug_auto_use_arena(0)
        try:
            got = device_call(lib, dev, fmt, use_all, x)
        finally:
            lib.dxtlt_debug_auto_use_arena(1)
        check_against_statement(fmt, use_all, n, got, want, route="one by one")
        check_against_statement(fmt, use_all, n, device_call(lib, dev, fmt, use_all, x), want)      # and the arena is back


def host_call(lib, fmt, use_all, x, est):
    out = np.full(x.size + 2 * A.GUARD, GUARD_FILL, dtype=np.uint8)
    src = np.array(x)
    norm, mode, split, err = C.c_uint8(0xEE), C.c_uint8(0xEE), C.c_bool(False), C.c_uint32(99)
    f = getattr(lib, f"dxtlt_transform_bc{fmt}_auto_with_normalization")
    rc = f(src.ctypes.data, out.ctypes.data + A.GUARD, x.size, est, use_all, C.byref(norm), C.byref(mode), C.byref(split), C.byref(err))
    assert rc == A.OK and err.value == 0, lib.dxtlt_last_error()
    assert np.array_equal(src, x) and (out[:A.GUARD] == GUARD_FILL).all() and (out[A.GUARD + x.size:] == GUARD_FILL).all()
    return (norm.value, mode.value, int(split.value)), out[A.GUARD:A.GUARD + x.size]


@pytest.mark.parametrize("fmt,use_all", DEPTHS)
def test_host_call_with_the_builtin_estimator(lib, dev, oracle, fmt, use_all):
    """equals the device call, downloads no section and makes no callback"""
    builtin = lib.dxtlt_builtin_size_estimator()
    for n, kind in ((4097, "cycle"), (2, "solids"), (513, "none")):
        x, want = A.case(fmt, kind, n, use_all)
        on_device = device_call(lib, dev, fmt, use_all, x)
        choice, out = host_call(lib, fmt, use_all, x, builtin)
        assert A.last_estimation(lib) == (0, 0)
        assert A.last_totals(lib) == on_device[2] == want[2] and A.last(lib) == on_device[3]
        assert choice == on_device[0] == want[0] and np.array_equal(out, on_device[1]) and np.array_equal(out, want[1])


@pytest.mark.parametrize("use_all", [False, True])
def test_bc2_host_call_with_a_callers_estimator(lib, dev, oracle, use_all):
    """one max_compressed_size(len / 4), then the 12 / 24 candidates in order, each shown len / 4 bytes: the choice and the bytes of
    the statement with that estimator; without a normalisable block the plain auto call's 4 / 8 calls"""
    for kind, calls in (("cycle", 24 if use_all else 12), ("none", 8 if use_all else 4)):
        x = A.blocks(2, kind, 1025)
        log = []
        est, py_estimate = cabi.make_estimator("zlib", log)
        want = A.call_statement(2, use_all, x, estimate=lambda b: py_estimate(bytes(b)))
        choice, out = host_call(lib, 2, use_all, x, C.cast(C.pointer(est), C.c_void_p))
        assert log == [x.size // 4] * calls
        assert choice == want[0] and np.array_equal(out, want[1])


SCRIPTED_BLOCKS = (2, 3, 513)                    # a lone pair, an odd count, one tile and a block: the smallest of each


@pytest.mark.parametrize("use_all", [False, True])
def test_bc2_callers_estimator_failures_skip_and_survivors_win(lib, dev, oracle, use_all):
    """BC2's callback route under a scripted estimator, against the statement: every candidate is transformed and shown, a failing
    estimate skips its candidate and is no error of the call, and the fold is strict `<` from (None, Variant1, split) with the
    maximum size.  The statement has no failing estimate of its own: one is the answer SIZE_MAX, which under that fold never wins."""
    from oracle import oracle_c

    for n in SCRIPTED_BLOCKS:
        x = A.blocks(2, "cycle", n)
        bufs, any_normalized = A.normalized_buffers(2, x)
        assert any_normalized
        a, b = A.colour_span(2, x.size)
        secs = [((norm, int(v), int(sc)), cabi.section_key(oracle_c.transform("bc2", bufs[norm], v, split_colour=bool(sc))[a:b]))
                for norm, v, sc in A.candidates(2, use_all)]
        assert len(secs) == (24 if use_all else 12)

        def run(table, default, want_choice, what):
            log, cpu_log = [], []
            est = cabi.scripted_estimator(table, default, log)
            cpu = cabi.scripted_estimate(table, default, cpu_log)

            def skipping(buf):
                try:
                    return cpu(buf)
                except cabi.ScriptedFailure:
                    return A.U64_MAX

            want = A.call_statement(2, use_all, x, estimate=skipping)
            choice, out = host_call(lib, 2, use_all, x, C.cast(C.pointer(est), C.c_void_p))     # rc == 0, out_estimator_error == 0
            assert choice == want[0] == want_choice, (n, what, choice, want[0], want_choice)
            assert np.array_equal(out, want[1]), (n, what)
            assert [key[0] for key in log] == [x.size // 4] * len(secs), (n, what)               # failing candidates included
            assert log == cpu_log == [key for _c, key in secs], (n, what)

        run({}, ("fail", 9), (A.NONE, 1, 1), "all fail")
        for norm in range(3):                          # every estimate fails but one of this mode, which answers one below the maximum
            cand, key = secs[norm * len(secs) // 3 + norm]
            first = next(c for c, k in secs if k == key)       # (at two blocks the split and the unsplit section hold the same bytes)
            assert first[0] == norm
            run({key: cabi.SIZE_MAX - 1}, ("fail", 9), first, ("lone survivor", cand))
        run({}, 7, secs[0][0], "all equal")


def test_bc2_a_failing_max_compressed_size_is_reported_and_writes_nothing(lib, dev, oracle):
    x = A.blocks(2, "cycle", 513)
    log = []
    est, _py = cabi.make_estimator("fail_max", log)
    out = np.full(x.size + 2 * A.GUARD, GUARD_FILL, dtype=np.uint8)
    src = np.array(x)
    for use_all in (False, True):
        norm, mode, split, err = C.c_uint8(0xEE), C.c_uint8(0xEE), C.c_bool(False), C.c_uint32(99)
        rc = lib.dxtlt_transform_bc2_auto_with_normalization(src.ctypes.data, out.ctypes.data + A.GUARD, x.size, C.cast(C.pointer(est), C.c_void_p),
                                                             use_all, C.byref(norm), C.byref(mode), C.byref(split), C.byref(err))
        assert rc == 5 and err.value == 41, (rc, err.value, lib.dxtlt_last_error())              # DXTLT_E_ESTIMATOR, the callback's code
        assert b"max_compressed_size" in lib.dxtlt_last_error()
        assert (out == GUARD_FILL).all() and np.array_equal(src, x) and log == []
        assert (norm.value, mode.value, split.value) == (0xEE, 0xEE, False)


def test_a_capturing_stream_is_refused(lib, dev, oracle):
    import torch

    x, want = A.case(1, "cycle", 513, False)
    src, dst = Guarded(dev, x.size, 0, x), Guarded(dev, x.size)
    norm, mode, split = C.c_uint8(0xEE), C.c_uint8(0xEE), C.c_bool(False)
    a = torch.arange(64, dtype=torch.uint8, device=dev)
    b = torch.zeros_like(a)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.dxtlt_transform_bc1_auto_with_normalization_device(src.ptr, dst.ptr, x.size, False, stream(), C.byref(norm), C.byref(mode),
                                                                    C.byref(split))
        error = lib.dxtlt_last_error()
        b.copy_(a)
    assert rc == A.E_ARGUMENT and b"capturable" in error and norm.value == 0xEE
    graph.replay()                                                  # the capture is still alive, and nothing was enqueued into it
    torch.cuda.synchronize()
    assert torch.equal(a, b) and (dst.bytes() == GUARD_FILL).all()
    check_against_statement(1, False, 513, device_call(lib, dev, 1, False, x), want)       # a later ordinary call still works


@pytest.mark.parametrize("fmt", [1, 2])
def test_python_wrapper_on_tensors(pkg, lib, dev, oracle, fmt):
    import torch

    from dxt_lossless_transform_amd import estimator, normalize

    x, want = A.case(fmt, "cycle", 4097, False)
    d_x = torch.from_numpy(np.array(x)).to(dev)
    d_y = torch.empty_like(d_x)
    f = normalize.transform_bc1_auto_with_normalization if fmt == 1 else normalize.transform_bc2_auto_with_normalization
    got = f(d_x, d_y)
    if fmt == 1:
        got = (got.color_normalization_mode, got.decorrelation_mode, got.split_colour_endpoints)
    assert (int(got[0]), int(got[1]), int(got[2])) == want[0]
    assert estimator.last_auto_totals() == want[2]
    torch.cuda.synchronize()
    assert np.array_equal(d_y.cpu().numpy(), want[1]) and np.array_equal(d_x.cpu().numpy(), x)
    y = np.zeros(x.size, dtype=np.uint8)                            # host buffers, no estimator given: the built-in one
    host = f(np.array(x), y)
    if fmt == 1:
        host = (host.color_normalization_mode, host.decorrelation_mode, host.split_colour_endpoints)
    assert (int(host[0]), int(host[1]), int(host[2])) == want[0] and np.array_equal(y, want[1])
    assert estimator.last_auto_estimation() == (0, 0)
