"""The built-in size estimator on the MI355X (csrc/estimate_kernels.hip, include/dxtlt_estimator.h) against its CPU statement
(tests/estimator_ref.py, docs/ESTIMATOR.md): every number exact.  And the auto transforms with it: the same choice and bytes
as the CPU loop over the same estimator (oracle/oracle_auto.py, tests/bc45_ref.py) and as the callback route, with no section
downloaded and no callback made."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import bc45_ref
import cabi
import estimator_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = R.W


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E(pkg):
    from dxt_lossless_transform_amd import estimator

    assert estimator.version() == R.VERSION
    return estimator


@pytest.fixture(scope="module")
def lib(pkg):
    """a handle of this file's own: argument types in the tests' cabi.DltSizeEstimator"""
    l = C.CDLL(pkg._lib.lib_path())
    vp, sz, b, i32 = C.c_void_p, C.c_size_t, C.c_bool, C.c_int32
    u8p, bp, estp = C.POINTER(C.c_uint8), C.POINTER(C.c_bool), C.POINTER(cabi.DltSizeEstimator)
    for n in ("bc1", "bc2"):
        getattr(l, f"dxtlt_transform_{n}_auto").argtypes = [vp, vp, sz, estp, b, u8p, bp, C.POINTER(C.c_uint32)]
        getattr(l, f"dxtlt_transform_{n}_auto_device").argtypes = [vp, vp, sz, b, vp, u8p, bp]
    l.dxtlt_transform_bc3_auto.argtypes = [vp, vp, sz, estp, b, u8p, bp, bp, C.POINTER(C.c_uint32)]
    l.dxtlt_transform_bc3_auto_device.argtypes = [vp, vp, sz, b, vp, u8p, bp, bp]
    for n in ("bc4", "bc5"):
        getattr(l, f"dxtlt_transform_{n}_auto").argtypes = [vp, vp, sz, estp, bp]
        getattr(l, f"dxtlt_transform_{n}_auto_device").argtypes = [vp, vp, sz, b, vp, bp]
    l.dxtlt_builtin_size_estimator.restype = estp
    l.dxtlt_estimate_size.argtypes, l.dxtlt_estimate_size.restype = [vp, sz, C.POINTER(C.c_uint64)], i32
    l.dxtlt_debug_auto_last_estimation.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    l.dxtlt_debug_auto_last_estimation.restype = None
    l.dxtlt_debug_auto_use_arena.argtypes, l.dxtlt_debug_auto_use_arena.restype = [i32], None
    l.dxtlt_dds_transform_auto.argtypes, l.dxtlt_dds_transform_auto.restype = [vp, sz, vp, sz, estp, b], i32
    l.dxtlt_dds_untransform.argtypes, l.dxtlt_dds_untransform.restype = [vp, sz, vp, sz], i32
    l.dxtlt_last_error.restype = C.c_char_p
    l.dxtlt_set_auto_estimator_threads.argtypes, l.dxtlt_set_auto_estimator_threads.restype = [i32], None
    return l


def golden(fmt):
    return np.fromfile(os.path.join(ROOT, "tests", "golden", f"r2-256-{fmt}.payload.bin"), dtype=np.uint8)


def texture_like(nbytes, seed):
    """5000 bytes of the reference's BC1 test texture over and over (a period that divides neither a window nor a 16-byte line), one
    byte in 97 replaced: long repeats, broken at random -- the estimate is about 0.11 of the length"""
    rng = np.random.default_rng(seed)
    g = golden("bc1")[:5000]
    x = np.tile(g, nbytes // g.size + 1)[:nbytes].copy()
    at = rng.integers(0, nbytes, nbytes // 97)
    x[at] = rng.integers(0, 256, at.size, dtype=np.uint8)
    return x


def period(n, p):
    return np.resize(np.arange(1, p + 1, dtype=np.uint8) * 37, n)


LENGTHS = sorted(set(list(range(0, 131)) + list(range(W - 4, W + 5)) + list(range(2 * W - 4, 2 * W + 5))))


# ---- dxtlt_estimate_size_device ------------------------------------------------------------------------------------
def test_single_section_every_short_length_and_window_edge(E, dev):
    import torch

    rng = np.random.default_rng(0xE571)
    pool = rng.integers(0, 4, 2 * W + 64, dtype=np.uint8)      # four byte values: matches everywhere
    d = torch.from_numpy(pool).to(dev)
    for n in LENGTHS:
        assert E.estimate_size(d[:n]) == R.estimate(pool[:n]), n
    for n in (5, 130, W + 1):
        assert R.estimate(pool[:n]) == R.estimate_loop(pool[:n])
    assert E.estimate_size(torch.from_numpy(np.frombuffer(R.WORKED_VECTOR, dtype=np.uint8).copy()).to(dev)) == R.WORKED_ESTIMATE


@pytest.mark.parametrize("off", [1, 2, 4, 8, 15])
def test_single_section_pointer_offsets(E, dev, off):
    import torch

    rng = np.random.default_rng(off)
    pool = np.concatenate([rng.integers(0, 3, 3 * W, dtype=np.uint8), period(W, 7)])
    d = torch.from_numpy(pool).to(dev)
    for n in (4, 17, 4096, W - 1, W, W + 3, 3 * W + 999):
        for o in (off, off + 16 * 5, off + W):
            assert E.estimate_size(d[o:o + n]) == R.estimate(pool[o:o + n]), (o, n)


def test_single_section_patterns(E, dev):
    import torch

    cases = [np.zeros(3 * W + 11, dtype=np.uint8)] + [period(2 * W + 5, p) for p in range(1, 10)]
    cases.append(R.colliding_grams())
    for k, x in enumerate(cases):
        want = R.estimate(x)
        assert E.estimate_size(torch.from_numpy(x).to(dev)) == want, k
    col = R.colliding_grams(256)
    assert R.estimate(col) == R.estimate_loop(col) and R.estimate(col) > col.size // 2      # b never counts as a match of a


@pytest.mark.parametrize("kind", ["random", "texture"])
def test_single_section_64_mib(E, dev, kind):
    import torch

    n = 64 << 20
    x = np.random.default_rng(64).integers(0, 256, n, dtype=np.uint8) if kind == "random" else texture_like(n, 65)
    want = R.estimate(x)
    d = torch.from_numpy(x).to(dev)
    assert E.estimate_size(d) == want
    assert E.estimate_size(d[3:n - 5]) == R.estimate(x[3:n - 5])
    if kind == "texture":
        assert want < n // 2                                      # the case has matches to count
        out = torch.zeros(1, dtype=torch.int64, device=dev)
        for lanes in (256, 512, 1024):                            # the result does not depend on the workgroup size
            E.estimate_sizes([d], out, shape=(lanes, R.W, R.BITS))
            assert int(out.item()) == want, lanes


@pytest.mark.parametrize("w,bits", [(32768, 13), (16384, 13), (8192, 12)])
def test_other_window_and_table_sizes_of_the_bench_sweep(E, dev, w, bits):
    """the kernel instances tools/estimator_bench.py sweeps compute the same definition with their own constants"""
    import torch

    x = np.concatenate([texture_like(5 * W + 123, w), np.random.default_rng(bits).integers(0, 3, 2 * W + 7, dtype=np.uint8)])
    d = torch.from_numpy(x).to(dev)
    secs = [(0, x.size), (5, 3 * w + 2), (w - 1, w + 1), (17, 3)]
    out = torch.zeros(len(secs), dtype=torch.int64, device=dev)
    for lanes in (256, 1024):
        E.estimate_sizes([d[o:o + n] for o, n in secs], out, shape=(lanes, w, bits))
        assert out.cpu().tolist() == [R.estimate(x[o:o + n], w, bits) for o, n in secs], lanes
    with pytest.raises(Exception):
        E.estimate_sizes([d], out, shape=(1024, 4096, 11))        # not compiled in: refused, not approximated


# ---- dxtlt_estimate_sizes_device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 6, 10, 257])
def test_many_sections_in_one_call(E, dev, count):
    import torch

    rng = np.random.default_rng(count)
    pool = np.concatenate([rng.integers(0, 5, 6 * W, dtype=np.uint8), texture_like(4 * W, count)])
    d = torch.from_numpy(pool).to(dev)
    lens = [0, 1, 3, 4, 5, W - 1, W, W + 1, 2 * W + 77, 5 * W + 3]
    secs = []
    for k in range(count):
        n = lens[k % len(lens)] if k % 3 else int(rng.integers(0, 3 * W))
        o = int(rng.integers(0, pool.size - n + 1))
        secs.append((o, n))
    guard = 8
    out = torch.full((count + 2 * guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    E.estimate_sizes([d[o:o + n] for o, n in secs], out[guard:guard + count])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:guard] == 0x5A5A5A5A5A5A5A5A).all() and (got[guard + count:] == 0x5A5A5A5A5A5A5A5A).all()
    for k, (o, n) in enumerate(secs):
        assert int(got[guard + k]) == R.estimate(pool[o:o + n]), (k, o, n)


def test_every_head_residue_with_every_short_length_and_window_edge(E, dev):
    """The kernel's first and last vectors are masked by the pointer's residue mod 16 and by (residue + length) mod 16 together:
    all 16 residues with every length 0..40 and the lengths around one and two windows, in one table."""
    import torch

    pool = np.random.default_rng(0xD17).integers(0, 3, 2 * W + 32, dtype=np.uint8)      # three byte values: matches everywhere
    d = torch.from_numpy(pool).to(dev)
    assert d.data_ptr() % 16 == 0                                                        # h below is the pointer's residue
    short = list(range(0, 41))
    lengths = short + list(range(W - 3, W + 4)) + list(range(2 * W - 3, 2 * W + 4))
    secs = [(h, n) for n in lengths for h in range(16)]
    want = [R.estimate(pool[h:h + n]) for h, n in secs]
    assert len(secs) == 55 * 16 and all(w < n for (h, n), w in zip(secs, want) if n >= 16)  # matches are counted, not lengths alone
    guard = 8

    def check(count, shape):
        out = torch.full((count + 2 * guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        E.estimate_sizes([d[h:h + n] for h, n in secs[:count]], out[guard:guard + count], shape=shape)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:guard] == 0x5A5A5A5A5A5A5A5A).all() and (got[guard + count:] == 0x5A5A5A5A5A5A5A5A).all(), shape
        bad = [(secs[k], int(got[guard + k]), want[k]) for k in range(count) if int(got[guard + k]) != want[k]]
        assert not bad, (shape, len(bad), bad[:8])

    check(len(secs), None)
    for lanes in (256, 512):                                  # the other workgroup sizes: the same masks over another stride
        check(len(short) * 16, (lanes, W, R.BITS))


def test_host_pointer_call_and_vtable_callback(E, lib):
    est = lib.dxtlt_builtin_size_estimator().contents
    size = C.c_size_t(123)
    assert est.MaxCompressedSize(None, 1 << 20, C.byref(size)) == 0 and size.value == 0
    for k, x in enumerate([texture_like(3 * W + 5, 1), np.random.default_rng(2).integers(0, 2, 70_001, dtype=np.uint8), period(9, 2)]):
        want = R.estimate(x)
        assert E.estimate_size(x) == want, k
        assert E.estimate_size(x[1:]) == R.estimate(x[1:]), k
        got = C.c_size_t()
        assert est.EstimateCompressedSize(None, x.ctypes.data, x.size, None, 0, C.byref(got)) == 0
        assert got.value == want, k


# ---- auto ----------------------------------------------------------------------------------------------------------
def ref_callback_estimator(log):
    """a DltSizeEstimator of Python callbacks over estimator_ref: the callback route with the same numbers"""
    @cabi.MAXFN
    def max_fn(ctx, n, out):
        out[0] = 0
        return 0

    @cabi.ESTFN
    def est_fn(ctx, inp, n, scratch, scratch_len, out):
        log.append(n)
        out[0] = R.estimate(C.string_at(inp, n) if n else b"")
        return 0

    est = cabi.DltSizeEstimator(None, max_fn, est_fn)
    est._keep = (max_fn, est_fn)
    return est


def wrapped_builtin_estimator(lib, log):
    """a copy of the built-in vtable whose function pointers are Python wrappers around the library's own: the same estimator,
    but not recognisable by identity -- every estimate is a dxtlt_estimate_size call from INSIDE the auto call"""
    inner = lib.dxtlt_builtin_size_estimator().contents
    inner_max, inner_est = inner.MaxCompressedSize, inner.EstimateCompressedSize

    @cabi.MAXFN
    def max_fn(ctx, n, out):
        return inner_max(ctx, n, out)

    @cabi.ESTFN
    def est_fn(ctx, inp, n, scratch, scratch_len, out):
        log.append(n)
        return inner_est(ctx, inp, n, scratch, scratch_len, out)

    est = cabi.DltSizeEstimator(None, max_fn, est_fn)
    est._keep = (max_fn, est_fn)
    return est


def last_estimation(lib):
    a, b = C.c_uint64(), C.c_uint64()
    lib.dxtlt_debug_auto_last_estimation(C.byref(a), C.byref(b))
    return a.value, b.value


def auto_inputs(fmt, oracle):
    block = 8 if fmt in ("bc1", "bc4") else 16
    xs = []
    if fmt in ("bc1", "bc2", "bc3"):
        xs.append(golden(fmt))
        xs += [oracle.generate_test_data(fmt, n) for n in (1, 3, 129, 4097, 70_001)]
    rng = np.random.default_rng(len(fmt) * 131 + block)
    for n in (2, 255, 8191, 33_333):
        x = rng.integers(0, 256, n * block, dtype=np.uint8).reshape(n, block)
        x[:, :block // 2] = (np.arange(n)[:, None] // (7 + n % 5) + np.arange(block // 2)[None, :] * 3) & 0xFF   # endpoints that repeat
        if fmt in ("bc2", "bc3"):
            x[:, 8:12] = x[:, 0:4] * 5 + 1                        # their colour endpoints too, or every colour section estimates alike
        xs.append(x.reshape(-1))
    return xs


def call_auto(lib, fmt, x, est, use_all, device=None):
    """-> (choice, output bytes, rc); choice = (variant, split_alpha, split_colour) as oracle_auto counts, BC4/5: split_endpoints"""
    import torch

    m, a, c = C.c_uint8(0xEE), C.c_bool(), C.c_bool()
    if device is None:
        out = np.full(x.size, 0xA5, dtype=np.uint8)
        f = getattr(lib, f"dxtlt_transform_{fmt}_auto")
        if fmt in ("bc4", "bc5"):
            rc = f(x.ctypes.data, out.ctypes.data, x.size, est, C.byref(a))
        elif fmt == "bc3":
            rc = f(x.ctypes.data, out.ctypes.data, x.size, est, use_all, C.byref(m), C.byref(a), C.byref(c), None)
        else:
            rc = f(x.ctypes.data, out.ctypes.data, x.size, est, use_all, C.byref(m), C.byref(c), None)
        got = out
    else:
        guard = 64
        d_in = torch.from_numpy(x).to(device)
        d_out = torch.full((x.size + 2 * guard,), 0xA5, dtype=torch.uint8, device=device)
        o = d_out[guard:guard + x.size]
        stream = torch.cuda.current_stream().cuda_stream
        f = getattr(lib, f"dxtlt_transform_{fmt}_auto_device")
        if fmt in ("bc4", "bc5"):
            rc = f(d_in.data_ptr(), o.data_ptr(), x.size, use_all, stream, C.byref(a))
        elif fmt == "bc3":
            rc = f(d_in.data_ptr(), o.data_ptr(), x.size, use_all, stream, C.byref(m), C.byref(a), C.byref(c))
        else:
            rc = f(d_in.data_ptr(), o.data_ptr(), x.size, use_all, stream, C.byref(m), C.byref(c))
        torch.cuda.synchronize()
        whole = d_out.cpu().numpy()
        assert (whole[:guard] == 0xA5).all() and (whole[guard + x.size:] == 0xA5).all(), "wrote outside the output"
        assert np.array_equal(d_in.cpu().numpy(), x), "the input changed"
        got = whole[guard:guard + x.size]
    choice = bool(a.value) if fmt in ("bc4", "bc5") else (m.value, int(a.value) if fmt == "bc3" else 0, int(c.value))
    return choice, got, rc


def cpu_auto(fmt, x, use_all, oracle):
    if fmt in ("bc4", "bc5"):
        split = bc45_ref.auto_choice(fmt, x, lambda b: R.estimate(b))
        return bool(split), bc45_ref.transform(fmt, x, split)
    from oracle import oracle_auto

    choice, out, _ = oracle_auto.transform_auto(fmt, x, R.estimate, use_all)
    return tuple(int(v) for v in choice), np.asarray(out)


CASES = [(f, u) for f in ("bc1", "bc2", "bc3") for u in (False, True)] + [("bc4", False), ("bc5", False)]


@pytest.mark.parametrize("fmt,use_all", CASES)
def test_auto_with_the_builtin_estimator(lib, dev, oracle, fmt, use_all):
    builtin = lib.dxtlt_builtin_size_estimator()
    for k, x in enumerate(auto_inputs(fmt, oracle)):
        want_choice, want = cpu_auto(fmt, x, use_all, oracle)
        # the existing entry point, the built-in estimator: nothing downloaded, nothing called
        choice, got, rc = call_auto(lib, fmt, x, builtin, use_all)
        assert rc == 0, lib.dxtlt_last_error()
        assert last_estimation(lib) == (0, 0), k
        assert choice == want_choice and np.array_equal(got, want), (k, choice, want_choice)
        # the same entry point, the same estimator behind Python callbacks: today's route
        log = []
        choice, got, rc = call_auto(lib, fmt, x, C.pointer(ref_callback_estimator(log)), use_all)
        assert rc == 0, lib.dxtlt_last_error()
        down, calls = last_estimation(lib)
        assert down > 0 and calls > 0 and calls == len(log) + 1, (k, down, calls, len(log))
        assert choice == want_choice and np.array_equal(got, want), (k, "callbacks", choice, want_choice)
        # the built-in estimator behind wrapped pointers: its host-pointer call runs inside the auto call, which keeps the input
        # in this thread's staging buffers the whole time -- also with the arena switched off, where every candidate is one more
        # transform FROM that input, and with the estimator on several threads (one of them the calling thread).
        # dxtlt_debug_auto_use_arena(0) reaches caller-supplied estimators too: (1, 0) is the sequential one-transform-per-candidate
        # callback flow (without the arena there is no parallel flow, whatever the thread count)
        for threads, arena_on in ((1, 1), (1, 0), (4, 1)) if k % 2 == 0 or k < 2 else ((1, 1),):
            log = []
            lib.dxtlt_set_auto_estimator_threads(threads)
            lib.dxtlt_debug_auto_use_arena(arena_on)
            try:
                choice, got, rc = call_auto(lib, fmt, x, C.pointer(wrapped_builtin_estimator(lib, log)), use_all)
            finally:
                lib.dxtlt_set_auto_estimator_threads(1)
                lib.dxtlt_debug_auto_use_arena(1)
            assert rc == 0, lib.dxtlt_last_error()
            assert len(log) > 0 and last_estimation(lib)[1] > 0
            assert choice == want_choice and np.array_equal(got, want), (k, "wrapped built-in", threads, arena_on, choice, want_choice)
        # device pointers
        choice, got, rc = call_auto(lib, fmt, x, None, use_all, device=dev)
        assert rc == 0, lib.dxtlt_last_error()
        assert last_estimation(lib) == (0, 0), k
        assert choice == want_choice and np.array_equal(got, want), (k, "device", choice, want_choice)
        if k % 3 == 1:        # as if the candidate arena could not be allocated: one full transform per candidate
            lib.dxtlt_debug_auto_use_arena(0)
            try:
                for device in (None, dev):
                    choice, got, rc = call_auto(lib, fmt, x, builtin, use_all, device=device)
                    assert rc == 0 and last_estimation(lib) == (0, 0)
                    assert choice == want_choice and np.array_equal(got, want), (k, "no arena", device, choice, want_choice)
            finally:
                lib.dxtlt_debug_auto_use_arena(1)


@pytest.mark.parametrize("fmt,use_all", CASES)
def test_auto_device_on_empty_and_sub_vector_buffers(lib, dev, fmt, use_all):
    builtin = lib.dxtlt_builtin_size_estimator()
    block = 8 if fmt in ("bc1", "bc4") else 16
    for n in (0, 1):
        x = np.random.default_rng(n).integers(0, 256, n * block, dtype=np.uint8)
        host = call_auto(lib, fmt, x, builtin, use_all)
        device = call_auto(lib, fmt, x, None, use_all, device=dev)
        assert host[2] == 0 and device[2] == 0
        assert host[0] == device[0] and np.array_equal(host[1], device[1]), n
    assert call_auto(lib, fmt, np.zeros(block + 1, dtype=np.uint8), None, use_all, device=dev)[2] == 1       # DXTLT_E_INVALID_LENGTH


@pytest.mark.parametrize("fmt", ["bc4", "bc5", "bc1"])
def test_auto_device_calls_of_one_thread_on_two_streams(lib, dev, fmt):
    """The call returns with its winning transform still enqueued, and the candidate arena belongs to the thread's next auto call:
    a second call on another stream, issued at once, must not disturb the first one's output (nor the other way round)."""
    import torch

    block = 8 if fmt in ("bc1", "bc4") else 16
    n = (48 << 20) // block
    rng = np.random.default_rng(n)
    xs = []
    for flat in (True, False):
        x = rng.integers(0, 256, n * block, dtype=np.uint8).reshape(n, block)
        if flat:
            x[:, 0] = 7                                         # the two buffers favour different settings
        else:
            x[:, :2] = rng.integers(0, 4, (n, 1), dtype=np.uint8) * np.array([[17, 91]], dtype=np.uint8)
        xs.append(x.reshape(-1))
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    d_out = [torch.zeros_like(t) for t in d_in]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()

    def call(i):
        m, a, c = C.c_uint8(), C.c_bool(), C.c_bool()
        f = getattr(lib, f"dxtlt_transform_{fmt}_auto_device")
        args = (d_in[i].data_ptr(), d_out[i].data_ptr(), xs[i].size, False, streams[i].cuda_stream)
        rc = f(*args, C.byref(a)) if fmt != "bc1" else f(*args, C.byref(m), C.byref(c))
        assert rc == 0, lib.dxtlt_last_error()
        return (m.value, c.value) if fmt == "bc1" else a.value

    # reference results: each call alone, waited for
    alone = []
    for i in (0, 1):
        choice = call(i)
        torch.cuda.synchronize()
        alone.append((choice, d_out[i].clone()))
        d_out[i].zero_()
    torch.cuda.synchronize()
    for _ in range(3):
        choices = [call(0), call(1)]                            # back to back, nothing waited for in between
        torch.cuda.synchronize()
        for i in (0, 1):
            assert choices[i] == alone[i][0]
            assert torch.equal(d_out[i], alone[i][1]), (fmt, i)
            d_out[i].zero_()


def test_auto_device_refuses_a_capturing_stream(lib, dev, E):
    """The readback makes the call uncapturable: an error at once -- nothing enqueued, nothing waited for -- and the capture is
    still alive afterwards (a synchronising call would have invalidated it)."""
    import torch

    x = torch.from_numpy(golden("bc1")).to(dev)
    y = torch.zeros_like(x)
    pre = torch.zeros_like(x)
    counters = torch.zeros(1, dtype=torch.int64, device=dev)
    E.estimate_sizes([x], counters)                                  # warm-up outside capture (module load)
    torch.cuda.synchronize()
    want = int(counters.item())
    counters.zero_()
    m, c = C.c_uint8(), C.c_bool()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.dxtlt_transform_bc1_auto_device(x.data_ptr(), y.data_ptr(), x.numel(), False, stream, C.byref(m), C.byref(c))
        out = C.c_uint64()
        rc2 = E._l().dxtlt_estimate_size_device(x.data_ptr(), x.numel(), stream, C.byref(out))
        E.estimate_sizes([x], counters)                              # enqueue-only: capturable
    assert rc == 2 and rc2 == 2
    assert b"capturable" in lib.dxtlt_last_error()
    assert torch.equal(y, pre)
    graph.replay()
    torch.cuda.synchronize()
    assert int(counters.item()) == want == R.estimate(golden("bc1"))


# ---- DDS -----------------------------------------------------------------------------------------------------------
def test_dds_auto_with_the_builtin_estimator_round_trips(lib, oracle):
    """the reference's integration-test DDS (one BC1 block behind a 128-byte header, integration_test.rs:28-57) and the three
    256 x 256 test textures behind their headers"""
    builtin = lib.dxtlt_builtin_size_estimator()
    d = bytearray(136)
    d[0:4] = b"DDS "
    struct.pack_into("<I", d, 4, 124)
    struct.pack_into("<I", d, 8, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000)
    struct.pack_into("<II", d, 0x0C, 4, 4)
    struct.pack_into("<I", d, 0x50, 0x4)
    d[0x54:0x58] = b"DXT1"
    d[0x80:0x88] = bytes([0x00, 0xF8, 0xE0, 0x07, 0, 0, 0, 0])
    files = [np.frombuffer(bytes(d), dtype=np.uint8).copy()]
    for fmt in ("bc1", "bc2", "bc3"):
        header = np.fromfile(os.path.join(ROOT, "tests", "golden", f"r2-256-{fmt}.header.bin"), dtype=np.uint8)
        files.append(np.concatenate([header, golden(fmt)]))
    for k, f in enumerate(files):
        t = np.zeros_like(f)
        assert lib.dxtlt_dds_transform_auto(f.ctypes.data, f.size, t.ctypes.data, t.size, builtin, bool(k & 1)) == 0, lib.dxtlt_last_error()
        assert last_estimation(lib) == (0, 0)
        assert t[:4].tobytes() != b"DDS "
        if k:
            fmt = ("bc1", "bc2", "bc3")[k - 1]
            off = f.size - golden(fmt).size
            _, want = cpu_auto(fmt, f[off:], bool(k & 1), oracle)
            assert np.array_equal(t[off:], want), fmt
        r = np.zeros_like(f)
        assert lib.dxtlt_dds_untransform(t.ctypes.data, t.size, r.ctypes.data, r.size) == 0
        assert np.array_equal(r, f), k
