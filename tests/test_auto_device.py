"""The all-on-device auto transforms (include/dxtlt_estimator.h, auto_on_device in csrc/auto_transform.cpp) where a choice and
its bytes alone say little: at every pointer alignment, candidate total by candidate total (dxtlt_debug_auto_last_totals against
the CPU loop over tests/estimator_ref.py), from several host threads at once, and after the thread's resources were released.
Every comparison is integer or byte equality."""
import ctypes as C
import threading

import numpy as np
import pytest

import bc45_ref
import estimator_ref as R
from test_estimator_gpu import CASES, E, auto_inputs, call_auto, cpu_auto, dev, last_estimation, lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16, "bc4": 8, "bc5": 16}
COUNTS = (1, 2, 3, 17, 129, 4097)     # an odd BC1 last block, less than a workgroup, 2-byte aligned split sections, several windows
IN_OFFSETS = (0, 1, 4, 8, 15)         # 4: the payload behind a DX10 DDS header starts at byte 148
OUT_OFFSETS = (0, 3)
GUARD = 64


def repeating_blocks(fmt, n, seed=0):
    """n blocks like auto_inputs': random index bytes behind endpoints that repeat, so the candidates differ.  The first endpoint
    byte moves slowly, the second every few blocks with another period: sections that keep them apart estimate smaller."""
    block = BLOCK[fmt]
    rng = np.random.default_rng(seed * 7919 + n * 31 + block + len(fmt) + int(fmt[2]))
    x = rng.integers(0, 256, n * block, dtype=np.uint8).reshape(n, block)
    k = np.arange(n)
    x[:, :block // 2] = (k[:, None] // (7 + n % 5) + np.arange(block // 2)[None, :] * 3) & 0xFF
    x[:, 1] = (k // 3 * 29) & 0xFF
    if fmt in ("bc2", "bc3"):                                   # colour endpoints: bytes 8..11
        x[:, 8:12] = ((k[:, None] // (5 + n % 3)) * np.array([[1, 0, 3, 0]]) + np.array([[0, 0x21, 0, 0x43]])) & 0xFF
    if fmt == "bc5":                                            # green endpoints: bytes 8, 9
        x[:, 8] = (k // 11) & 0xFF
        x[:, 9] = (k // 2 * 53) & 0xFF
    return x.reshape(-1)


def candidates_of(fmt, use_all):
    if fmt in ("bc4", "bc5"):
        return [False, True]
    from oracle import oracle_auto

    return oracle_auto.test_order(fmt, use_all)


_cpu = {}


def cpu_answer(fmt, x, use_all, oracle):
    """-> (totals in candidate order, choice, bytes): the CPU loop, once per input.  The totals are this file's own sum over the
    sections each candidate's CPU transform shows the estimator; choice and bytes are what the suite's CPU auto loops return, and
    the two must agree (strict `<`: the first smallest total)."""
    key = (fmt, use_all, x.size, hash(x.tobytes()))
    if key not in _cpu:
        n = x.size // BLOCK[fmt]
        totals = []
        for cand in candidates_of(fmt, use_all):
            if fmt in ("bc4", "bc5"):
                t = bc45_ref.transform(fmt, x, cand)
                secs = bc45_ref.endpoint_sections(fmt, n)                       # BC4 endpoints; BC5 red, then green
            else:
                v, sa, sc = cand
                t = np.asarray(oracle.transform(fmt, x, v, sc, sa))
                secs = {"bc1": [(0, x.size // 2)], "bc2": [(x.size // 2, x.size // 2 + x.size // 4)],
                        "bc3": [(0, 2 * n), (x.size // 2, x.size // 2 + 4 * n)]}[fmt]   # BC3: alpha endpoints, then colour
            totals.append(sum(R.estimate(t[a:b]) for a, b in secs))
        choice, out = cpu_auto(fmt, x, use_all, oracle)
        pick = candidates_of(fmt, use_all)[int(np.argmin(totals))]              # argmin: the first of equal totals
        assert choice == (bool(pick) if fmt in ("bc4", "bc5") else tuple(pick)), (fmt, use_all, totals, choice)
        _cpu[key] = (totals, choice, out)
    return _cpu[key]


def last_totals(lib):
    buf = (C.c_uint64 * 16)()
    n = lib.dxtlt_debug_auto_last_totals(buf, 16)
    return [int(v) for v in buf[:n]]


@pytest.fixture(scope="module")
def L(lib):
    lib.dxtlt_debug_auto_last_totals.argtypes = [C.POINTER(C.c_uint64), C.c_int32]
    lib.dxtlt_debug_auto_last_totals.restype = C.c_int32
    lib.dxtlt_estimate_size_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.dxtlt_estimate_size_device.restype = C.c_int32
    lib.dxtlt_release_thread_resources.argtypes, lib.dxtlt_release_thread_resources.restype = [], None
    return lib


def device_call(lib, fmt, d_in, d_out, nbytes, use_all, stream):
    """the C call on raw device pointers -> (rc, choice as cpu_auto counts it)"""
    m, a, c = C.c_uint8(0xEE), C.c_bool(), C.c_bool()
    f = getattr(lib, f"dxtlt_transform_{fmt}_auto_device")
    if fmt in ("bc4", "bc5"):
        rc = f(d_in, d_out, nbytes, use_all, stream, C.byref(a))
        return rc, bool(a.value)
    if fmt == "bc3":
        rc = f(d_in, d_out, nbytes, use_all, stream, C.byref(m), C.byref(a), C.byref(c))
    else:
        rc = f(d_in, d_out, nbytes, use_all, stream, C.byref(m), C.byref(c))
    return rc, (m.value, int(a.value) if fmt == "bc3" else 0, int(c.value))


def expected_count(fmt, use_all):
    return 2 if fmt in ("bc4", "bc5") else (8 if fmt == "bc3" else 4) * (2 if use_all else 1)


# ---- A: every pointer alignment --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,use_all", CASES)
def test_device_auto_at_every_pointer_alignment(L, dev, oracle, fmt, use_all):
    """d_input at byte 0, 1, 4, 8 and 15 of an allocation, d_output at byte 0 and 3 inside a guard band: rc 0, the CPU loop's
    choice, bytes and totals, nothing outside the output written, the input unchanged, nothing downloaded -- also with the
    candidate arena switched off.  (BC1-3 off a 16-byte boundary were refused with DXTLT_E_DEVICE before the no-arena route was
    taken for them.)"""
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    for n in COUNTS:
        x = repeating_blocks(fmt, n)
        want_totals, want_choice, want = cpu_answer(fmt, x, use_all, oracle)
        assert len(want_totals) == expected_count(fmt, use_all)
        plan = [(i, o, 1) for i in IN_OFFSETS for o in OUT_OFFSETS] + [(i, o, 0) for i in (1, 15) for o in OUT_OFFSETS]
        for i, o, arena_on in plan:
            pad = np.full(i + x.size + 16, 0x3C, dtype=np.uint8)
            pad[i:i + x.size] = x
            d_in = torch.from_numpy(pad).to(dev)
            d_out = torch.full((GUARD + o + x.size + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
            p_in, p_out = d_in.data_ptr() + i, d_out.data_ptr() + GUARD + o
            assert d_in.data_ptr() % 256 == 0 and p_in % 16 == i            # the offset is the pointer's residue
            L.dxtlt_debug_auto_use_arena(arena_on)
            try:
                rc, choice = device_call(L, fmt, p_in, p_out, x.size, use_all, stream)
            finally:
                L.dxtlt_debug_auto_use_arena(1)
            at = (fmt, use_all, n, i, o, arena_on)
            assert rc == 0, (at, rc, L.dxtlt_last_error())
            assert last_estimation(L) == (0, 0), at
            assert last_totals(L) == want_totals, at
            torch.cuda.synchronize()
            whole = d_out.cpu().numpy()
            assert choice == want_choice, (at, choice, want_choice)
            assert np.array_equal(whole[GUARD + o:GUARD + o + x.size], want), at
            assert (whole[:GUARD + o] == 0xA5).all() and (whole[GUARD + o + x.size:] == 0xA5).all(), at
            assert np.array_equal(d_in.cpu().numpy(), pad), at


@pytest.mark.parametrize("fmt,use_all,n,i,o", [("bc1", False, 4097, 4, 3), ("bc3", True, 129, 15, 0), ("bc5", False, 17, 1, 3)])
def test_python_wrapper_on_torch_slices(L, E, dev, oracle, fmt, use_all, n, i, o):
    """estimator.transform_auto on slices of device tensors: the same settings as the C call's out-parameters"""
    import torch

    x = repeating_blocks(fmt, n)
    want_totals, want_choice, want = cpu_answer(fmt, x, use_all, oracle)
    d_in = torch.full((i + x.size + 5,), 0x3C, dtype=torch.uint8, device=dev)
    d_in[i:i + x.size] = torch.from_numpy(x).to(dev)
    d_out = torch.full((GUARD + o + x.size + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    src, dst = d_in[i:i + x.size], d_out[GUARD + o:GUARD + o + x.size]
    assert src.data_ptr() % 16 == i and dst.data_ptr() % 16 == o
    settings = E.transform_auto(fmt, src, dst, use_all)
    assert E.last_auto_estimation() == (0, 0) and E.last_auto_totals() == want_totals
    torch.cuda.synchronize()
    whole = d_out.cpu().numpy()
    assert np.array_equal(whole[GUARD + o:GUARD + o + x.size], want)
    assert (whole[:GUARD + o] == 0xA5).all() and (whole[GUARD + o + x.size:] == 0xA5).all()
    assert torch.equal(src, torch.from_numpy(x).to(dev))
    rc, choice = device_call(L, fmt, src.data_ptr(), dst.data_ptr(), x.size, use_all, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and choice == want_choice
    if fmt in ("bc4", "bc5"):
        assert type(settings).__name__ == f"Bc{fmt[2]}TransformSettings" and settings.split_endpoints is choice
    else:
        got = (int(settings.decorrelation_mode), int(getattr(settings, "split_alpha_endpoints", False)), int(settings.split_colour_endpoints))
        assert type(settings).__name__ == f"Bc{fmt[2]}TransformSettings" and got == choice


# ---- B: the totals, candidate by candidate ---------------------------------------------------------------------------
def totals_inputs(fmt, oracle):
    return auto_inputs(fmt, oracle) + [repeating_blocks(fmt, n) for n in COUNTS]


@pytest.mark.parametrize("fmt,use_all", CASES)
def test_per_candidate_totals(L, dev, oracle, fmt, use_all):
    """What the argmin is taken over: a wrong arena offset, counter index or stale counter shows here even where it leaves the
    choice alone.  Device pointers and the host-pointer call given the built-in estimator, the arena on and off."""
    builtin = L.dxtlt_builtin_size_estimator()
    count = expected_count(fmt, use_all)
    picks = set()
    for k, x in enumerate(totals_inputs(fmt, oracle)):
        want_totals, want_choice, want = cpu_answer(fmt, x, use_all, oracle)
        assert len(want_totals) == count
        # conditions on the inputs, for the CPU loop alone to meet
        if x.size // BLOCK[fmt] >= 129:
            assert len(set(want_totals)) >= 2, (k, want_totals)
        picks.add(int(np.argmin(want_totals)))
        for arena_on in (1, 0):
            for device in (dev, None):
                L.dxtlt_debug_auto_use_arena(arena_on)
                try:
                    choice, got, rc = call_auto(L, fmt, x, builtin, use_all, device=device)
                finally:
                    L.dxtlt_debug_auto_use_arena(1)
                at = (k, arena_on, "device" if device is not None else "host")
                assert rc == 0, (at, L.dxtlt_last_error())
                assert last_totals(L) == want_totals, at
                assert choice == want_choice and np.array_equal(got, want), at
                assert last_estimation(L) == (0, 0), at
    assert picks - {0}, "no input of this format makes a candidate other than the first win"
    # no totals after a call that compared none: an empty buffer, a refused length, the callback route
    x = repeating_blocks(fmt, 3)
    assert call_auto(L, fmt, x, None, use_all, device=dev)[2] == 0 and len(last_totals(L)) == count
    assert call_auto(L, fmt, x[:0], None, use_all, device=dev)[2] == 0 and last_totals(L) == []
    assert call_auto(L, fmt, x, None, use_all, device=dev)[2] == 0 and len(last_totals(L)) == count
    assert call_auto(L, fmt, x[:x.size - 1], None, use_all, device=dev)[2] == 1 and last_totals(L) == []
    assert call_auto(L, fmt, x, builtin, use_all)[2] == 0 and len(last_totals(L)) == count
    from test_estimator_gpu import ref_callback_estimator

    assert call_auto(L, fmt, x, C.pointer(ref_callback_estimator([])), use_all)[2] == 0 and last_totals(L) == []


# ---- C: several host threads, and a thread whose resources were released ------------------------------------------
THREADS = [("bc1", False, 4097, 4), ("bc3", True, 33_333, 0), ("bc5", False, 129, 0), ("bc2", True, 4097, 0)]


def test_four_host_threads_at_once(L, dev, oracle):
    """The arena, the counter block and the upload stage are per thread: four threads, each on a stream and an input of its own
    (one of them 4 bytes off a 16-byte boundary), 20 calls back to back, every fifth an estimate of its own data -- every
    result is that thread's CPU answer."""
    import torch

    jobs = []
    for t, (fmt, use_all, n, off) in enumerate(THREADS):
        x = repeating_blocks(fmt, n, seed=t + 1)
        totals, choice, want = cpu_answer(fmt, x, use_all, oracle)
        d_in = torch.zeros(off + x.size, dtype=torch.uint8, device=dev)
        d_in[off:] = torch.from_numpy(x).to(dev)
        jobs.append(dict(fmt=fmt, use_all=use_all, x=x, off=off, totals=totals, choice=choice, whole=R.estimate(x), d_in=d_in,
                         d_want=torch.from_numpy(want).to(dev), d_out=torch.zeros(x.size, dtype=torch.uint8, device=dev),
                         stream=torch.cuda.Stream(dev)))
        assert (d_in.data_ptr() + off) % 16 == off
    assert len({j["choice"] if isinstance(j["choice"], tuple) else (j["choice"],) for j in jobs}) >= 2
    torch.cuda.synchronize()
    start = threading.Barrier(len(jobs))
    failures = []

    def work(t, j):
        try:
            with torch.cuda.stream(j["stream"]):
                stream = j["stream"].cuda_stream
                p_in = j["d_in"].data_ptr() + j["off"]
                start.wait()
                for call in range(20):
                    if call % 5 == 4:
                        got = C.c_uint64()
                        rc = L.dxtlt_estimate_size_device(p_in, j["x"].size, stream, C.byref(got))
                        assert rc == 0 and got.value == j["whole"], (t, call, rc, got.value, j["whole"])
                        continue
                    j["d_out"].fill_(0xA5)
                    rc, choice = device_call(L, j["fmt"], p_in, j["d_out"].data_ptr(), j["x"].size, j["use_all"], stream)
                    assert rc == 0, (t, call, rc, L.dxtlt_last_error())
                    assert last_totals(L) == j["totals"], (t, call)
                    assert last_estimation(L) == (0, 0), (t, call)
                    assert choice == j["choice"], (t, call, choice)
                    assert torch.equal(j["d_out"], j["d_want"]), (t, call)
                assert torch.equal(j["d_in"][j["off"]:].cpu(), torch.from_numpy(j["x"])), t
        except BaseException as e:          # noqa: BLE001  (reported from the main thread)
            start.abort()
            failures.append((t, repr(e)))
        finally:
            L.dxtlt_release_thread_resources()

    threads = [threading.Thread(target=work, args=(t, j)) for t, j in enumerate(jobs)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not failures, failures


def test_auto_after_the_thread_resources_were_released(L, dev, oracle):
    """a large buffer, then a small one (the arena is grow-only), dxtlt_release_thread_resources, both again, then an estimate of
    host memory: everything as in the first run"""
    builtin_inputs = [("bc3", True, repeating_blocks("bc3", 33_333)), ("bc3", True, repeating_blocks("bc3", 3)),
                      ("bc4", False, repeating_blocks("bc4", 33_333)), ("bc1", False, repeating_blocks("bc1", 3))]

    def run():
        res = []
        for fmt, use_all, x in builtin_inputs:
            choice, got, rc = call_auto(L, fmt, x, None, use_all, device=dev)
            assert rc == 0, L.dxtlt_last_error()
            res.append((choice, got.tobytes(), last_totals(L)))
        return res

    first = run()
    for (fmt, use_all, x), (choice, got, totals) in zip(builtin_inputs, first):
        want_totals, want_choice, want = cpu_answer(fmt, x, use_all, oracle)
        assert totals == want_totals and choice == want_choice and got == want.tobytes()
    L.dxtlt_release_thread_resources()
    assert run() == first
    x = builtin_inputs[0][2]
    out = C.c_uint64()
    assert L.dxtlt_estimate_size(x.ctypes.data, x.size, C.byref(out)) == 0 and out.value == R.estimate(x)
    L.dxtlt_release_thread_resources()
    assert L.dxtlt_estimate_size(x.ctypes.data, x.size, C.byref(out)) == 0 and out.value == R.estimate(x)
    assert run() == first
