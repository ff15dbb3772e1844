"""BC3's auto transform with block normalisation on the device (include/dxtlt_auto_normalize.h), held to the CPU statement of
tests/auto_normalize_bc3_ref.py: the candidate kernel's 20 / 32 sections byte for byte, the whole device call -- choice, output
bytes, the 96 / 192 totals and what it waited for and launched --, the routes without the arena, the host calls (the callback route
under a scripted estimator included), a capturing stream and the Python wrapper.
Every comparison is exact equality; every buffer the library writes lies between 256 guard bytes."""
import ctypes as C

import numpy as np
import pytest

import auto_normalize_bc3_ref as B
import auto_normalize_ref as A
import cabi
from test_auto_normalize_gpu import GUARD_FILL, Guarded, stream

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 255, 256, 257, 513, 1025)     # one block per lane: around one and two workgroups; odd counts put the alpha
                                                 # sections off 16-byte boundaries
CALL_BLOCKS = (1, 2, 4097, 20001)                # 20 001: alpha sections of 40 002 bytes (two estimator windows, the second short),
                                                 # colour sections of 80 004 bytes (three windows)


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return B.load(pkg)


def device_call(lib, dev, use_all, x, in_off=0):
    """(choice, output bytes, totals, last) of one device call; the input is checked to be unchanged"""
    import torch

    src, dst = Guarded(dev, x.size, in_off, x), Guarded(dev, x.size)
    outs = B.Outs()
    rc = lib.dxtlt_transform_bc3_auto_with_normalization_device(src.ptr, dst.ptr, x.size, use_all, stream(), *outs.refs())
    assert rc == B.OK, lib.dxtlt_last_error()
    last, totals = A.last(lib), B.last_totals(lib)
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), x), "the input was written"
    return outs.choice(), dst.bytes(), totals, last


def check_against_statement(use_all, n, got, want, route="arena"):
    choice, out, totals, last = got
    want_choice, want_out, want_totals, any_normalized = want
    assert choice == want_choice, (n, choice, want_choice)
    assert totals == want_totals, (n, [k for k, (a, b) in enumerate(zip(totals, want_totals)) if a != b][:4])
    assert np.array_equal(out, want_out), (n, int(np.nonzero(out != want_out)[0][0]))
    fused = 24 if use_all else 12
    if not any_normalized:
        assert last == [2, 0, 0, 0], (n, last)
    elif route == "arena":
        assert last == [2, 1, 2, 1], (n, last)                  # one candidate kernel; 20 / 32 sections: two estimator launches
    else:                                                       # one fused transform per colour section, one estimate per section
        assert last == [2, fused, fused + 8, 1], (n, last)


# ---- the candidate kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_all", [False, True])
def test_candidate_kernel_bytes(lib, dev, oracle, use_all):
    """every one of the 20 / 32 sections == the statement; the guards around the arena and the input are untouched"""
    import torch

    hook = lib.dxtlt_debug_bc3_auto_normalization_candidates_into_device
    runs = []
    for n in COUNTS:
        x, want = B.arena_case(use_all, n)
        src, arena = Guarded(dev, x.size, 0, x), Guarded(dev, want.size, 0, None, B.FILL)
        assert hook(use_all, src.ptr, x.size, arena.ptr, want.size, stream()) == B.OK, (n, lib.dxtlt_last_error())
        runs.append((n, x, want, src, arena))
    torch.cuda.synchronize()
    for n, x, want, src, arena in runs:
        got = arena.bytes()
        for key, off, length in B.sections(use_all, n):
            bad = np.nonzero(got[off:off + length] != want[off:off + length])[0]
            name = f"alpha mode {key[1]}, split {key[2]}" if key[0] == "a" else f"colour mode {key[1]}, variant {key[2]}, split {key[3]}"
            assert bad.size == 0, f"{n} blocks, section ({name}): {bad.size} bytes differ, first at {int(bad[0]) if bad.size else -1}"
        assert np.array_equal(src.bytes(), x), "the input was written"


def test_candidate_hook_refusals_write_nothing(lib, dev, oracle):
    import torch

    x, want = B.arena_case(False, 513)
    src, arena = Guarded(dev, x.size, 0, x), Guarded(dev, want.size, 0, None, B.FILL)
    hook, s = lib.dxtlt_debug_bc3_auto_normalization_candidates_into_device, stream()
    assert hook(False, src.ptr, x.size - 8, arena.ptr, want.size, s) == B.E_ARGUMENT
    for off in (1, 4, 8):
        assert hook(False, src.ptr + off, x.size - 16, arena.ptr, want.size, s) == B.E_ARGUMENT, off
        assert hook(False, src.ptr, x.size - 16, arena.ptr + off, want.size - off, s) == B.E_ARGUMENT, off
    assert hook(False, src.ptr, x.size, arena.ptr, want.size - 1, s) == B.E_ARGUMENT and b"arena" in lib.dxtlt_last_error()
    assert hook(True, src.ptr, x.size, arena.ptr, want.size, s) == B.E_ARGUMENT              # all modes: 112 bytes per block
    assert hook(False, None, x.size, arena.ptr, want.size, s) == B.E_ARGUMENT
    assert hook(False, src.ptr, x.size, None, want.size, s) == B.E_ARGUMENT
    older = lib.dxtlt_debug_auto_normalization_candidates_into_device                        # keeps refusing format 3
    assert older(3, False, src.ptr, x.size, arena.ptr, want.size, s) == B.E_ARGUMENT
    torch.cuda.synchronize()
    assert (arena.bytes() == B.FILL).all()
    assert hook(False, src.ptr, x.size, arena.ptr, want.size, s) == B.OK                      # and the hook still works
    torch.cuda.synchronize()
    assert np.array_equal(arena.bytes(), want)


# ---- the whole device call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_all", [False, True])
@pytest.mark.parametrize("kind", list(B.KINDS))
def test_device_call_equals_the_statement(lib, dev, oracle, kind, use_all):
    for n in CALL_BLOCKS:
        x, want = B.case(kind, n, use_all)
        got = device_call(lib, dev, use_all, x)
        check_against_statement(use_all, n, got, want)
        assert A.last_estimation(lib) == (0, 0)
        assert want[3] == (kind != "none") or n <= 2                 # (the first blocks of a kind need not be normalisable ones)
        if not want[3]:
            assert got[3] == [2, 0, 0, 0] and len(got[2]) == (16 if use_all else 8)
            src, dst = Guarded(dev, x.size, 0, x), Guarded(dev, x.size)
            mode, split_alpha, split_colour = C.c_uint8(0xEE), C.c_bool(False), C.c_bool(False)
            assert lib.dxtlt_transform_bc3_auto_device(src.ptr, dst.ptr, x.size, use_all, stream(), C.byref(mode), C.byref(split_alpha),
                                                       C.byref(split_colour)) == B.OK
            assert B.last_totals(lib) == got[2]
            assert (0, 0, mode.value, int(split_alpha.value), int(split_colour.value)) == got[0] and np.array_equal(dst.bytes(), got[1])
        else:
            assert got[3][3] == 1 and len(got[2]) == (192 if use_all else 96)


def test_every_mode_wins_on_the_device(lib, dev, oracle):
    won_alpha, won_colour = set(), set()
    for kind in B.KINDS:
        x, want = B.case(kind, 4097, False)
        got = device_call(lib, dev, False, x)
        check_against_statement(False, 4097, got, want)
        won_alpha.add(got[0][0])
        won_colour.add(got[0][1])
    assert won_alpha == {0, 1, 2, 3} and won_colour == {0, 1, 2}


def test_empty_input(lib, dev):
    for use_all in (False, True):
        outs = B.Outs()
        assert lib.dxtlt_transform_bc3_auto_with_normalization_device(None, None, 0, use_all, stream(), *outs.refs()) == B.OK
        mode, split_alpha, split_colour = C.c_uint8(0xEE), C.c_bool(False), C.c_bool(False)
        assert lib.dxtlt_transform_bc3_auto_device(None, None, 0, use_all, stream(), C.byref(mode), C.byref(split_alpha),
                                                   C.byref(split_colour)) == B.OK
        assert outs.choice() == (0, 0, mode.value, int(split_alpha.value), int(split_colour.value))


# ---- the other routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_all", [False, True])
def test_unaligned_input_and_no_arena_make_the_same_choice(lib, dev, oracle, use_all):
    for n, kind in ((4097, "cycle"), (513, "opaque"), (513, "none")):
        x, want = B.case(kind, n, use_all)
        for off in (1, 4, 8):
            got = device_call(lib, dev, use_all, x, in_off=off)
            check_against_statement(use_all, n, got, want, route="one by one")
        lib.dxtlt_debug_auto_use_arena(0)
        try:
            got = device_call(lib, dev, use_all, x)
        finally:
            lib.dxtlt_debug_auto_use_arena(1)
        check_against_statement(use_all, n, got, want, route="one by one")
        check_against_statement(use_all, n, device_call(lib, dev, use_all, x), want)      # and the arena is back


def host_call(lib, use_all, x, est, want_rc=B.OK):
    out = np.full(x.size + 2 * B.GUARD, GUARD_FILL, dtype=np.uint8)
    src = np.array(x)
    outs, err = B.Outs(), C.c_uint32(99)
    rc = lib.dxtlt_transform_bc3_auto_with_normalization(src.ctypes.data, out.ctypes.data + B.GUARD, x.size, est, use_all, *outs.refs(),
                                                         C.byref(err))
    assert rc == want_rc, (rc, lib.dxtlt_last_error())
    assert np.array_equal(src, x) and (out[:B.GUARD] == GUARD_FILL).all() and (out[B.GUARD + x.size:] == GUARD_FILL).all()
    return outs, out[B.GUARD:B.GUARD + x.size], err.value


@pytest.mark.parametrize("use_all", [False, True])
def test_host_call_with_the_builtin_estimator(lib, dev, oracle, use_all):
    """equals the device call, downloads no section and makes no callback"""
    builtin = lib.dxtlt_builtin_size_estimator()
    for n, kind in ((4097, "cycle"), (2, "uniform"), (513, "none")):
        x, want = B.case(kind, n, use_all)
        on_device = device_call(lib, dev, use_all, x)
        outs, out, err = host_call(lib, use_all, x, builtin)
        assert err == 0 and A.last_estimation(lib) == (0, 0)
        assert B.last_totals(lib) == on_device[2] == want[2] and A.last(lib) == on_device[3]
        assert outs.choice() == on_device[0] == want[0] and np.array_equal(out, on_device[1]) and np.array_equal(out, want[1])


def shown_keys(use_all, x):
    """the (len, crc32) keys of the sections the callback route shows, in the order it shows them: per fused launch k (one per colour
    section) the alpha section k for k < 8, then colour section k"""
    secs = B.section_bytes(use_all, x)
    layout = [key for key, _off, _len in B.sections(use_all, x.size // 16)]
    order = []
    for k, colour_key in enumerate(layout[8:]):
        if k < 8:
            order.append(layout[k])
        order.append(colour_key)
    return order, {key: cabi.section_key(secs[key]) for key in layout}


@pytest.mark.parametrize("use_all", [False, True])
def test_host_call_with_a_callers_estimator(lib, dev, oracle, use_all):
    """every one of the 20 / 32 sections is shown once, len / 8 or len / 4 bytes each: the choice and the bytes of the statement with
    that estimator; without a normalisable block the plain auto call's callbacks"""
    x = B.blocks("cycle", 1025)
    log = []
    est, py_estimate = cabi.make_estimator("crc", log)
    want = B.call_statement(use_all, x, estimate=lambda b: py_estimate(bytes(b)))
    outs, out, err = host_call(lib, use_all, x, C.cast(C.pointer(est), C.c_void_p))
    order, keys = shown_keys(use_all, x)
    assert log == [keys[key] for key in order] and len(log) == (32 if use_all else 20)
    assert err == 0 and outs.choice() == want[0] and np.array_equal(out, want[1])
    x = B.blocks("none", 1025)
    log.clear()
    want = B.call_statement(use_all, x, estimate=lambda b: py_estimate(bytes(b)))
    outs, out, err = host_call(lib, use_all, x, C.cast(C.pointer(est), C.c_void_p))
    assert not want[3] and err == 0 and outs.choice() == want[0] and np.array_equal(out, want[1])
    assert sorted({k[0] for k in log}) == [x.size // 8, x.size // 4]


@pytest.mark.parametrize("use_all", [False, True])
def test_callers_estimator_failures_skip_and_survivors_win(lib, dev, oracle, use_all):
    """the callback route under a scripted estimator, against the statement: a failing estimate skips every candidate that uses its
    section and is no error of the call; the fold is strict `<` from the defaults with the maximum size."""
    for n in (27, 513):                              # 27: the smallest count that holds the opaque classes, which tell modes 1 - 3 apart
        x = B.blocks("cycle", n)
        order, keys = shown_keys(use_all, x)
        assert len(set(keys.values())) == len(keys), "the sections of this data are pairwise different"
        layout = [key for key, _off, _len in B.sections(use_all, n)]
        cands = B.candidates(use_all)

        def run(table, default, want_choice, what):
            log = []
            est = cabi.scripted_estimator(table, default, log)
            answer = lambda key: table.get(keys[key], default)
            failed = {k for k, key in enumerate(layout) if isinstance(answer(key), tuple)}
            choice, _totals = B.fold(use_all, [0 if k in failed else answer(key) for k, key in enumerate(layout)], failed)
            assert choice == want_choice, (n, what, choice, want_choice)
            outs, out, err = host_call(lib, use_all, x, C.cast(C.pointer(est), C.c_void_p))
            assert err == 0 and outs.choice() == want_choice, (n, what, outs.choice(), want_choice)
            am, cm, v, sa, sc = want_choice
            assert np.array_equal(out, oracle.transform("bc3", oracle.normalize_bc3_blocks(x, am, cm), v, split_colour=bool(sc),
                                                        split_alpha=bool(sa))), (n, what)
            assert log == [keys[key] for key in order], (n, what)                              # failing sections included, each once

        run({}, ("fail", 9), (0, 0, 1, 1, 1), "all fail")
        run({}, 7, cands[0], "all equal")
        for c in (cands[0], cands[len(cands) // 2 + 3], cands[-1]):          # one alpha and one colour section survive: their candidate
            am, cm, v, sa, sc = c
            table = {keys[("a", am, sa)]: 5, keys[("c", cm, v, sc)]: 0}
            run(table, ("fail", 9), c, ("lone survivor", c))
        # every colour section fails: no candidate survives whatever the alpha sections answer
        run({keys[key]: 3 for key in layout[:8]}, ("fail", 9), (0, 0, 1, 1, 1), "no colour section")
        # one failing colour section only: its candidates are skipped, the rest compete
        failing = ("c", cands[0][1], cands[0][2], cands[0][4])
        table = {keys[failing]: ("fail", 9)}
        run(table, 7, next(c for c in cands if ("c", c[1], c[2], c[4]) != failing), "first colour section fails")


def test_a_failing_max_compressed_size_is_reported_and_writes_nothing(lib, dev, oracle):
    x = B.blocks("cycle", 513)
    log = []
    est, _py = cabi.make_estimator("fail_max", log)
    for use_all in (False, True):
        outs, out, err = host_call(lib, use_all, x, C.cast(C.pointer(est), C.c_void_p), want_rc=B.E_ESTIMATOR)
        assert err == 41 and b"max_compressed_size" in lib.dxtlt_last_error()                 # the callback's code
        assert (out == GUARD_FILL).all() and log == [] and outs.untouched()
    # the second query (len / 4) failing is reported the same way
    calls = []

    @cabi.MAXFN
    def max_fn(ctx, n, out_ptr):
        calls.append(n)
        if n == x.size // 4:
            return 43
        out_ptr[0] = n + 64
        return 0

    second = cabi.DltSizeEstimator(None, max_fn, est._keep[1])
    outs, out, err = host_call(lib, False, x, C.cast(C.pointer(second), C.c_void_p), want_rc=B.E_ESTIMATOR)
    assert err == 43 and calls == [x.size // 8, x.size // 4] and (out == GUARD_FILL).all() and outs.untouched()


def test_a_capturing_stream_is_refused(lib, dev, oracle):
    import torch

    x, want = B.case("cycle", 513, False)
    src, dst = Guarded(dev, x.size, 0, x), Guarded(dev, x.size)
    outs = B.Outs()
    a = torch.arange(64, dtype=torch.uint8, device=dev)
    b = torch.zeros_like(a)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.dxtlt_transform_bc3_auto_with_normalization_device(src.ptr, dst.ptr, x.size, False, stream(), *outs.refs())
        error = lib.dxtlt_last_error()
        b.copy_(a)
    assert rc == B.E_ARGUMENT and b"capturable" in error and outs.untouched()
    graph.replay()                                                  # the capture is still alive, and nothing was enqueued into it
    torch.cuda.synchronize()
    assert torch.equal(a, b) and (dst.bytes() == GUARD_FILL).all()
    check_against_statement(False, 513, device_call(lib, dev, False, x), want)       # a later ordinary call still works


def test_python_wrapper_on_tensors(pkg, lib, dev, oracle):
    import torch

    from dxt_lossless_transform_amd import estimator, normalize

    x, want = B.case("cycle", 4097, False)
    d_x = torch.from_numpy(np.array(x)).to(dev)
    d_y = torch.empty_like(d_x)
    got = normalize.transform_bc3_auto_with_normalization(d_x, d_y)
    assert tuple(int(v) for v in got) == want[0]
    assert estimator.last_auto_totals() == want[2]
    torch.cuda.synchronize()
    assert np.array_equal(d_y.cpu().numpy(), want[1]) and np.array_equal(d_x.cpu().numpy(), x)
    y = np.zeros(x.size, dtype=np.uint8)                            # host buffers, no estimator given: the built-in one
    host = normalize.transform_bc3_auto_with_normalization(np.array(x), y)
    assert tuple(int(v) for v in host) == want[0] and np.array_equal(y, want[1])
    assert estimator.last_auto_estimation() == (0, 0)
