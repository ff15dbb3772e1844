"""The pixel auto transform on the MI355X (csrc/pixel_auto_api.cpp, pixel_auto_kernels.hip; include/dxtlt_pixels.h) against its
CPU statement: tests/pixels_ref.py for every candidate's bytes, tests/entropy_ref.py for the six totals and the pick."""
import ctypes as C

import numpy as np
import pytest

import entropy_ref as R
import pixels_auto_data as D
import pixels_ref

pytestmark = pytest.mark.gpu

GUARD = 256
PIXEL_COUNTS = [1, 15, 16, 17, 4095, 4096, 4097, 8192 + 1, 32768, 32768 + 7, 87381]


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    l = pixels_ref.declare(C.CDLL(pkg._lib.lib_path()))
    vp, sz, i32, b, u64p = C.c_void_p, C.c_size_t, C.c_int32, C.c_bool, C.POINTER(C.c_uint64)
    bp, u8p = C.POINTER(C.c_bool), C.POINTER(C.c_uint8)
    l.dxtlt_transform_pixels_auto_device.argtypes, l.dxtlt_transform_pixels_auto_device.restype = [vp, vp, sz, i32, vp, bp, u8p], i32
    l.dxtlt_transform_pixels_auto.argtypes = [vp, vp, sz, i32, C.POINTER(pixels_ref.Estimator), bp, u8p]
    l.dxtlt_transform_pixels_auto.restype = i32
    l.dxtlt_debug_pixels_auto_last_totals.argtypes, l.dxtlt_debug_pixels_auto_last_totals.restype = [u64p, i32], i32
    l.dxtlt_debug_auto_last_estimation.argtypes, l.dxtlt_debug_auto_last_estimation.restype = [u64p, u64p], None
    l.dxtlt_debug_auto_use_arena.argtypes, l.dxtlt_debug_auto_use_arena.restype = [i32], None
    l.dxtlt_builtin_entropy_estimator.restype = C.POINTER(pixels_ref.Estimator)
    l.dxtlt_estimate_entropy_size.argtypes, l.dxtlt_estimate_entropy_size.restype = [vp, sz, u64p], i32
    l.dxtlt_file_formats_enable_pixel_auto.argtypes, l.dxtlt_file_formats_enable_pixel_auto.restype = [b], None
    l.dxtlt_last_error.restype = C.c_char_p
    return l


@pytest.fixture(scope="module")
def sources():
    """87 381 pixels of two kinds per B: the mip chain of the r2-256 image (the first candidate wins) and random walks (the fourth)"""
    chain = np.ascontiguousarray(D.data_sets()[2][1])
    assert chain.shape == (87381, 4)
    out = {4: [chain, D.random_walks(4, 87381, 11)], 3: [np.ascontiguousarray(chain[:, :3]), D.random_walks(3, 87381, 12)]}
    for arrays in out.values():
        for a in arrays:
            a.setflags(write=False)
    return out


_REF = {}


def reference(key, flat, B):
    """(totals, pick, the pick's bytes) of the statement, computed once per input"""
    if key not in _REF:
        _REF[key] = R.auto(flat, B)
    return _REF[key]


def totals_of(lib):
    buf = (C.c_uint64 * 8)()
    n = lib.dxtlt_debug_pixels_auto_last_totals(buf, 8)
    return [int(v) for v in buf[:n]]


def estimation_of(lib):
    a, b = C.c_uint64(99), C.c_uint64(99)
    lib.dxtlt_debug_auto_last_estimation(C.byref(a), C.byref(b))
    return a.value, b.value


def device_auto(lib, dev, flat, B, in_off=0, out_off=0):
    """the device call on a d_input `in_off` and a d_output `out_off` bytes past a 256-byte boundary, d_output between guard bytes;
    returns ((decorrelate, layout), output bytes, totals) after checking the guards, the input and the round trip"""
    import torch

    n = flat.size
    src = torch.full((GUARD + in_off + n,), 0x11, dtype=torch.uint8, device=dev)
    src[GUARD + in_off:] = torch.from_numpy(flat.copy()).to(dev)
    before = src.clone()
    dst = torch.full((GUARD + out_off + n + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    dec, lay = C.c_bool(), C.c_uint8(9)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.dxtlt_transform_pixels_auto_device(src.data_ptr() + GUARD + in_off, dst.data_ptr() + GUARD + out_off, n, B, stream,
                                                C.byref(dec), C.byref(lay))
    assert rc == 0, lib.dxtlt_last_error()
    totals = totals_of(lib)
    assert estimation_of(lib) == (0, 0)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:GUARD + out_off] == 0xEE).all() and (host[GUARD + out_off + n:] == 0xEE).all(), "guard bytes written"
    assert torch.equal(src, before), "input written"
    back = torch.zeros(n, dtype=torch.uint8, device=dev)
    got = dst[GUARD + out_off:GUARD + out_off + n].clone()
    assert lib.dxtlt_untransform_pixels_device(got.data_ptr(), back.data_ptr(), n, B, dec.value, lay.value, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy(), flat), "round trip"
    return (dec.value, lay.value), host[GUARD + out_off:GUARD + out_off + n].copy(), totals


@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("P", PIXEL_COUNTS)
def test_totals_choice_and_bytes_equal_the_statement_on_both_routes(lib, dev, sources, B, P):
    for k, px in enumerate(sources[B]):
        flat = np.ascontiguousarray(px[:P]).reshape(-1)
        totals, at, want = reference((B, P, k), flat, B)
        for arena in (1, 0):
            lib.dxtlt_debug_auto_use_arena(arena)
            try:
                choice, got, dev_totals = device_auto(lib, dev, flat, B)
            finally:
                lib.dxtlt_debug_auto_use_arena(1)
            assert dev_totals == totals, (k, arena, dev_totals, totals)
            assert choice == R.CANDIDATES[at], (k, arena)
            assert np.array_equal(got, want), (k, arena)


@pytest.mark.parametrize("B", [3, 4])
def test_pointer_residues(lib, dev, sources, B):
    """d_input at residues 0, 1, 8, 16 (off a 16-byte boundary: one transform per candidate) and d_output at 0, 3, 16"""
    P = 4097
    for k, px in enumerate(sources[B]):
        flat = np.ascontiguousarray(px[:P]).reshape(-1)
        totals, at, want = reference((B, P, k), flat, B)
        for in_off in (0, 1, 8, 16):
            for out_off in (0, 3, 16):
                choice, got, dev_totals = device_auto(lib, dev, flat, B, in_off, out_off)
                assert dev_totals == totals and choice == R.CANDIDATES[at], (k, in_off, out_off)
                assert np.array_equal(got, want), (k, in_off, out_off)


def test_the_pick_on_the_small_data_sets(lib, dev):
    """128 x 128 versions of the data sets of tests/test_entropy_estimator.py: the picks are 1, 1, 1, 4, 4, 4, 4"""
    picks = []
    for name, px in D.small_sets():
        B, flat = px.shape[1], px.reshape(-1)
        totals, at, want = reference(("small", name), flat, B)
        choice, got, dev_totals = device_auto(lib, dev, flat, B)
        assert dev_totals == totals and choice == R.CANDIDATES[at] and np.array_equal(got, want), name
        picks.append(at + 1)
    assert picks == [1, 1, 1, 4, 4, 4, 4]


@pytest.mark.parametrize("k", range(12))
def test_every_candidate_wins_strictly_on_both_routes(lib, dev, k):
    """the twelve inputs of pixels_auto_data.winner_sets: each of the six candidates is the one strict winner once per pixel size
    (held to the statement without a device by tests/test_pixels_batch_auto_gpu.py)"""
    name, B, px, winner = D.winner_sets()[k]
    flat = px.reshape(-1)
    totals, at, want = reference(("winner", name), flat, B)
    assert at == winner and all(totals[at] < t for i, t in enumerate(totals) if i != at), name
    for arena in (1, 0):
        lib.dxtlt_debug_auto_use_arena(arena)
        try:
            choice, got, dev_totals = device_auto(lib, dev, flat, B)
        finally:
            lib.dxtlt_debug_auto_use_arena(1)
        assert dev_totals == totals, (name, arena, dev_totals, totals)
        assert choice == R.CANDIDATES[winner], (name, arena)
        assert np.array_equal(got, want), (name, arena)


def test_empty_buffer_and_ties_keep_the_first_candidate(lib, dev):
    dec, lay = C.c_bool(False), C.c_uint8(9)
    assert lib.dxtlt_transform_pixels_auto_device(None, None, 0, 4, None, C.byref(dec), C.byref(lay)) == 0
    assert (dec.value, lay.value) == (True, 2) and totals_of(lib) == []
    flat = np.full(4 * 5000, 0x7F, dtype=np.uint8)                   # every candidate is constant planes or pixels... a tie at the top
    choice, got, totals = device_auto(lib, dev, flat, 4)
    want_totals, at, want = R.auto(flat, 4)
    assert totals == want_totals and choice == R.CANDIDATES[at] and np.array_equal(got, want)


@pytest.mark.parametrize("B", [3, 4])
def test_host_call_with_the_entropy_estimator_stays_on_the_device(lib, sources, B):
    for k, px in enumerate(sources[B]):
        flat = np.ascontiguousarray(px[:8192 + 1]).reshape(-1)
        totals, at, want = reference((B, 8192 + 1, k), flat, B)
        out = np.zeros_like(flat)
        dec, lay = C.c_bool(), C.c_uint8(9)
        rc = lib.dxtlt_transform_pixels_auto(flat.ctypes.data, out.ctypes.data, flat.size, B, lib.dxtlt_builtin_entropy_estimator(),
                                             C.byref(dec), C.byref(lay))
        assert rc == 0, lib.dxtlt_last_error()
        assert estimation_of(lib) == (0, 0) and totals_of(lib) == totals
        assert (dec.value, lay.value) == R.CANDIDATES[at] and np.array_equal(out, want)


@pytest.mark.parametrize("B", [3, 4])
def test_callback_route_calls_in_candidate_order(lib, sources, B):
    """Any other estimator: MaxCompressedSize once, then six EstimateCompressedSize calls of len bytes, candidate after candidate
    (the sixth on the input itself); with dxtlt_estimate_entropy_size behind the callback the choice is the device route's."""
    flat = np.ascontiguousarray(sources[B][1][:4097]).reshape(-1)
    totals, at, want = reference((B, 4097, 1), flat, B)
    outs = [pixels_ref.forward(flat, B, d, l) for d, l in R.CANDIDATES]
    seen, max_calls = [], []

    def max_size(_ctx, n, out):
        max_calls.append(n)
        out[0] = 0
        return 0

    def estimate(_ctx, inp, n, _scratch, _scratch_len, out):
        data = np.ctypeslib.as_array(C.cast(inp, C.POINTER(C.c_uint8)), shape=(n,)).copy()
        v = C.c_uint64()
        rc = lib.dxtlt_estimate_entropy_size(inp, n, C.byref(v))
        seen.append((n, data, v.value))
        out[0] = v.value
        return rc

    est = pixels_ref.Estimator(None, pixels_ref.MAX_SIZE_FN(max_size), pixels_ref.ESTIMATE_FN(estimate))
    out = np.zeros_like(flat)
    dec, lay = C.c_bool(), C.c_uint8(9)
    for arena in (1, 0):
        seen.clear()
        max_calls.clear()
        lib.dxtlt_debug_auto_use_arena(arena)
        try:
            rc = lib.dxtlt_transform_pixels_auto(flat.ctypes.data, out.ctypes.data, flat.size, B, C.byref(est), C.byref(dec), C.byref(lay))
        finally:
            lib.dxtlt_debug_auto_use_arena(1)
        assert rc == 0, lib.dxtlt_last_error()
        assert max_calls == [flat.size] and [n for n, _d, _v in seen] == [flat.size] * 6
        for i, (_n, data, v) in enumerate(seen):
            assert np.array_equal(data, outs[i]), i
            assert v == totals[i], i
        assert (dec.value, lay.value) == R.CANDIDATES[at] and np.array_equal(out, want)
        assert estimation_of(lib) == (5 * flat.size, 7) and totals_of(lib) == []
    # an estimator that answers `len` for everything: a tie, the first candidate stays
    counting, calls = pixels_ref.counting_estimator()
    rc = lib.dxtlt_transform_pixels_auto(flat.ctypes.data, out.ctypes.data, flat.size, B, C.byref(counting), C.byref(dec), C.byref(lay))
    assert rc == 0 and calls[0] == 7 and (dec.value, lay.value) == (True, 2)
    assert np.array_equal(out, outs[0])

    def failing(_ctx, _inp, _n, _scratch, _scratch_len, _out):
        return 77

    bad = pixels_ref.Estimator(None, pixels_ref.MAX_SIZE_FN(max_size), pixels_ref.ESTIMATE_FN(failing))
    assert lib.dxtlt_transform_pixels_auto(flat.ctypes.data, out.ctypes.data, flat.size, B, C.byref(bad), None, None) == 5


def test_a_capturing_stream_is_refused_with_nothing_written(lib, dev, sources):
    import torch

    flat = np.ascontiguousarray(sources[4][0][:4096]).reshape(-1)
    x = torch.from_numpy(flat.copy()).to(dev)
    y = torch.zeros_like(x)
    warm = torch.zeros_like(x)
    assert lib.dxtlt_transform_pixels_device(x.data_ptr(), warm.data_ptr(), x.numel(), 4, True, 2,
                                             torch.cuda.current_stream().cuda_stream) == 0          # module load outside the capture
    torch.cuda.synchronize()
    dec, lay = C.c_bool(False), C.c_uint8(9)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.dxtlt_transform_pixels_auto_device(x.data_ptr(), y.data_ptr(), x.numel(), 4, stream, C.byref(dec), C.byref(lay))
        marker = lib.dxtlt_transform_pixels_device(x.data_ptr(), warm.data_ptr(), x.numel(), 4, False, 0, stream)   # capturable
    assert rc == 2 and marker == 0
    assert b"capturable" in lib.dxtlt_last_error()
    assert (dec.value, lay.value) == (False, 9) and totals_of(lib) == []
    graph.replay()                                                    # the capture is still alive: nothing waited inside it
    torch.cuda.synchronize()
    assert int(y.abs().sum().item()) == 0
    assert torch.equal(warm, x)


def test_dds_switch(lib, sources):
    """Off: the fixed setting and no callback, as ever.  On: the header word carries the auto's choice, and the file comes back."""
    P = 128 * 64
    flat = np.ascontiguousarray(sources[4][1][:P]).reshape(-1)         # random walks: the fourth candidate wins
    totals, at, want = reference(("dds", 4), flat, 4)
    assert R.CANDIDATES[at] == (False, 2)
    dds = np.frombuffer(pixels_ref.dds_dx10(flat.tobytes(), 128, 64, 28), dtype=np.uint8).copy()
    off = dds.size - flat.size
    counting, calls = pixels_ref.counting_estimator()
    entropy = lib.dxtlt_builtin_entropy_estimator()
    lib.dxtlt_file_formats_enable_pixels(True)
    try:
        t = np.zeros_like(dds)
        for est in (C.byref(counting), entropy):
            assert lib.dxtlt_dds_transform_auto(dds.ctypes.data, dds.size, t.ctypes.data, t.size, est, False) == 0
            assert calls[0] == 0
            assert int(t[:4].view("<u4")[0]) == pixels_ref.header_word(pixels_ref.TF_RGBA8888, True, 2)
            assert np.array_equal(t[off:], pixels_ref.forward(flat, 4, True, 2))
        lib.dxtlt_file_formats_enable_pixel_auto(True)
        assert lib.dxtlt_dds_transform_auto(dds.ctypes.data, dds.size, t.ctypes.data, t.size, entropy, False) == 0, lib.dxtlt_last_error()
        assert int(t[:4].view("<u4")[0]) == pixels_ref.header_word(pixels_ref.TF_RGBA8888, *R.CANDIDATES[at])
        assert np.array_equal(t[off:], want) and np.array_equal(t[4:off], dds[4:off])
        assert totals_of(lib) == totals and estimation_of(lib) == (0, 0)
        back = np.zeros_like(dds)
        assert lib.dxtlt_dds_untransform(t.ctypes.data, t.size, back.ctypes.data, back.size) == 0
        assert np.array_equal(back, dds)
        # the caller's estimator is called when the switch is on: a tie keeps the first candidate
        assert lib.dxtlt_dds_transform_auto(dds.ctypes.data, dds.size, t.ctypes.data, t.size, C.byref(counting), False) == 0
        assert calls[0] == 7
        assert int(t[:4].view("<u4")[0]) == pixels_ref.header_word(pixels_ref.TF_RGBA8888, True, 2)
    finally:
        lib.dxtlt_file_formats_enable_pixel_auto(False)
        lib.dxtlt_file_formats_enable_pixels(False)
