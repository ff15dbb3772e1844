"""The fused candidate kernels of the pixel auto transforms -- pixel_candidates<3|4> (csrc/pixel_auto_kernels.hip) and
pixel_batch_candidates<3|4> (csrc/pixel_batch_kernels.hip), both DXTLT_PIXEL_CANDIDATES_TILE of csrc/pixel_tile_body.h -- held to
their statement BYTE FOR BYTE: candidate i of an arena or slice is tests/pixels_ref.py's forward for the i-th setting of
entropy_ref.CANDIDATES, and no other byte is written.  The calls themselves show these kernels to nothing but the entropy estimator,
which cannot see a permutation inside a 32 KiB window and rounds a few wrong bytes away (the first test below, no device needed);
here two test hooks run them into memory of the test's own: dxtlt_debug_pixels_auto_candidates_into_device and
dxtlt_debug_pixels_batch_candidates_device (include/dxtlt_pixels.h).

Every arena is device memory filled with 0xEE, 256 bytes of it at least in front of and behind every arena; U.arena_differences is
the one comparison: every slice equal to the statement, every other byte still the fill.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import entropy_ref as R
import pixels_batch_util as U

OK, E_LENGTH, E_ARGUMENT = 0, 1, 2
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return U.load(pkg)


# ---- inputs and their statement, computed once ----------------------------------------------------------------------------------------
_SINGLE, _BATCH = {}, {}


def single_input(P, B, seed=None):
    """(input bytes, the five candidates side by side) of `P` pixels: a smooth half and a random half (U.source_bytes)"""
    key = (P, B, seed)
    if key not in _SINGLE:
        flat = U.source_bytes([U.candidate_case(P, B, 0)], seed=P * 8 + B if seed is None else seed)[0][0]
        ref = U.candidates_of(flat, B)
        flat.setflags(write=False)
        ref.setflags(write=False)
        _SINGLE[key] = (flat, ref)
    return _SINGLE[key]


def batch_input(name):
    """(cases, input bytes per item, candidates per item) of a case list of pixels_batch_util"""
    if name not in _BATCH:
        cases = {"mixed": U.cases_candidates_mixed, "wide": U.cases_candidates_wide}[name]()
        flats = [pair[0] for pair in U.source_bytes(cases, seed=0xCA4D + len(cases))]
        _BATCH[name] = (cases, flats, [U.candidates_of(f, c[1]) for f, c in zip(flats, cases)])
    return _BATCH[name]


# ---- no device: what the new comparison sees and the totals cannot ------------------------------------------------------------------
OBSERVER_SEED = 1      # found by a search from 1 upwards: at this seed the flipped bit below keeps all four totals


@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("P", [4097, 8193])
def test_the_totals_are_blind_to_what_the_byte_comparison_reports(B, P):
    """Three wrong arenas a slip in DXTLT_PIXEL_CANDIDATES_TILE would write -- the two halves of a tile of one plane exchanged (lane
    indexing in plane_store / planes_of), planes 0 and 2 exchanged, one bit wrong in the first byte behind a tile seam (a wrong
    `prev`) -- leave the candidate's estimate, all the calls ever compare, where it was; U.arena_differences names each."""
    flat, ref = single_input(P, B, OBSERVER_SEED)
    n = P * B
    assert 3 * P <= U.WINDOW          # planes 0..2 of a candidate lie in its first window: a swap among them keeps the histogram

    def seen_and_hidden(mutated, i):
        assert not np.array_equal(mutated, ref)
        assert R.estimate(mutated[i * n:(i + 1) * n]) == R.estimate(ref[i * n:(i + 1) * n]), i      # the totals: blind
        for j in range(5):
            if j != i:
                assert np.array_equal(mutated[j * n:(j + 1) * n], ref[j * n:(j + 1) * n])
        arena = np.full(U.GUARD + 5 * n + U.GUARD, U.ARENA_FILL, dtype=np.uint8)
        arena[U.GUARD:U.GUARD + 5 * n] = mutated
        report = U.arena_differences(arena, [(U.GUARD, ref, "arena")])
        assert len(report) == 1 and "differ" in report[0], report                                     # the bytes: seen

    for i, (_dec, layout) in enumerate(R.CANDIDATES[:5]):
        if layout == R.INTERLEAVED:
            continue
        m = ref.copy()
        a = i * n + P                                                    # plane 1, tile 0
        m[a:a + 2048], m[a + 2048:a + 4096] = ref[a + 2048:a + 4096], ref[a:a + 2048]
        seen_and_hidden(m, i)
        m = ref.copy()
        a = i * n
        m[a:a + P], m[a + 2 * P:a + 3 * P] = ref[a + 2 * P:a + 3 * P], ref[a:a + P]
        seen_and_hidden(m, i)
    m = ref.copy()
    m[n + U.TILE] ^= 1                                                   # candidate 1, plane 0, the first byte of tile 1
    seen_and_hidden(m, 1)
    # and the helper's other half: a byte outside every slice
    arena = np.full(U.GUARD + 5 * n + U.GUARD, U.ARENA_FILL, dtype=np.uint8)
    arena[U.GUARD:U.GUARD + 5 * n] = ref
    assert U.arena_differences(arena, [(U.GUARD, ref, "arena")]) == []
    arena[U.GUARD + 5 * n] = 0
    report = U.arena_differences(arena, [(U.GUARD, ref, "arena")])
    assert len(report) == 1 and "outside" in report[0], report


# ---- no device: what the case lists reach ------------------------------------------------------------------------------------------------
LAST_LANE_COUNTS = [U.TILE + 1 - v for v in range(1, 16)]


def test_the_case_lists_reach_what_they_claim(lib):
    # the single kernel: every `valid` of the last lane, 16 = the vector arm, 1..15 the byte arm of plane_store
    assert {U.last_lane_valid(P) for P in LAST_LANE_COUNTS + [U.TILE + 1]} == set(range(1, 17))
    assert [U.last_lane_valid(P) for P in U.CANDIDATE_COUNTS] == [1, 15, 16, 1, 15, 16, 1, 1, 15]
    # tiles: one short, one full, a seam with a last tile of 1 pixel, three tiles with a last tile of 4095
    assert [(-(-P // U.TILE), (P - 1) % U.TILE + 1) for P in U.CANDIDATE_COUNTS[4:]] == [(1, 4095), (1, 4096), (2, 1), (3, 1), (3, 4095)]
    assert all((P * 3) % 16 != 0 for P in (1, 15, 17, 4095, 4097, 8193, 12287))       # B = 3: stage_in / stage_out have a byte tail
    # the mixed batch
    mixed = U.cases_candidates_mixed()
    assert len(mixed) == 40 and {c[1] for c in mixed} == {3, 4}
    assert {(c[0], c[1]) for c in mixed if c[0] not in (0, U.LONG_ITEM)} == {(P, B) for P in U.CANDIDATE_BATCH_COUNTS for B in (3, 4)}
    assert {(c[5], c[1]) for c in mixed} == {(r, B) for r in U.CANDIDATE_RESIDUES for B in (3, 4)}
    assert mixed[21][0] == 0 and 0 < 21 < len(mixed) - 1                               # an empty item in the middle
    at = [c[0] for c in mixed].index(U.LONG_ITEM)
    assert all(mixed[k][1] == 4 and (k == at or mixed[k][0] <= U.TILE) for k in (at - 1, at, at + 1))
    arms = U.lookup_arms(mixed)
    assert arms == {(3, 0, 0, 0): (1, 32), (4, 0, 0, 0): (9, 91)}                      # (the index names the owner, the bisection finds it)
    arr = U.fake_auto_items(mixed)
    assert [arr[k].d_input % 16 for k in range(40)] == [c[5] for c in mixed]
    items, chunks = U.auto_plan(lib, arr, 40)
    assert len(chunks) == 1 and chunks[0].candidate_launches == 2                      # both pixel sizes in one chunk
    lib.dxtlt_debug_batch_auto_arena_cap(U.CANDIDATE_CHUNK_CAP)
    try:
        cut_items, cut = U.auto_plan(lib, arr, 40)
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)
    assert len(cut) == 7 >= 3 and sum(ch.candidate_launches == 2 for ch in cut) >= 3
    assert [ch.item_count for ch in cut if ch.arena_bytes > U.CANDIDATE_CHUNK_CAP] == [1]      # the long item, alone
    assert sorted({it.chunk for it in cut_items}) == list(range(7))
    # the wide index, in one launch of 3-byte pixels
    wide = U.cases_candidates_wide()
    assert len(wide) == 300 and {c[1] for c in wide} == {3} and {c[5] for c in wide} == set(U.CANDIDATE_RESIDUES)
    _items, chunks = U.auto_plan(lib, U.fake_auto_items(wide), 300)
    assert len(chunks) == 1 and chunks[0].candidate_launches == 1
    as_batch = [(c[0], 4, 0, 1, 2, c[5], c[6]) for c in wide]                          # the same spans through the batch call's planner
    assert U.plan(lib, U.fake_items(as_batch), 300)[1][0].wide == 1
    assert U.lookup_arms(wide) == {(3, 0, 0, 0): (21, 621)}


def test_the_hooks_check_their_arguments_before_any_device_work(lib):
    """no device: made-up addresses, nothing is dereferenced"""
    single, batch = lib.dxtlt_debug_pixels_auto_candidates_into_device, lib.dxtlt_debug_pixels_batch_candidates_device
    src, arena = 0x7000_0000_0000, 0x7100_0000_0000
    assert single(src, 4 * 100 + 1, 4, arena, None) == E_LENGTH and single(src, 3 * 100 + 1, 3, arena, None) == E_LENGTH
    assert single(src, 400, 2, arena, None) == E_ARGUMENT and single(src, 0, 4, arena, None) == E_ARGUMENT
    assert single(None, 400, 4, arena, None) == E_ARGUMENT and single(src + 8, 400, 4, arena, None) == E_ARGUMENT
    assert single(src, 400, 4, None, None) == E_ARGUMENT
    mixed = U.cases_candidates_mixed()
    arr = U.fake_auto_items(mixed)
    _items, chunks = U.auto_plan(lib, arr, len(mixed))
    size = chunks[0].arena_bytes
    assert batch(arr, len(mixed), 1, arena, size, None) == E_ARGUMENT and b"chunk" in lib.dxtlt_last_error()
    assert batch(arr, len(mixed), 0, arena, size - 1, None) == E_ARGUMENT and b"arena" in lib.dxtlt_last_error()
    assert batch(arr, len(mixed), 0, None, size, None) == E_ARGUMENT
    assert batch(arr, 0, 0, arena, size, None) == E_ARGUMENT and batch(None, 3, 0, arena, size, None) == E_ARGUMENT
    arr[5].len += 1
    assert batch(arr, len(mixed), 0, arena, size, None) == E_LENGTH
    assert all((a.decorrelate, a.layout) == (0, 0) for a in arr[:len(mixed)])          # (fake_auto_items leaves them 0)


# ---- the single kernel -----------------------------------------------------------------------------------------------------------------
def run_single(lib, dev, jobs):
    """jobs: [(P, B, input offset inside a 128-byte line, arena residue)] -- every input and every arena of 5 * len bytes in one buffer
    each, between guard bytes; all launches, one synchronise, one comparison"""
    import torch

    data = [single_input(P, B) for P, B, _i, _a in jobs]
    arenas = U.Arenas(dev, [flat for flat, _ref in data], [j[2] for j in jobs], [j[3] for j in jobs], out_lengths=[ref.size for _f, ref in data])
    stream = torch.cuda.current_stream().cuda_stream
    for k, ((P, B, in_off, residue), (flat, _ref)) in enumerate(zip(jobs, data)):
        assert arenas.in_ptr(k) % U.LINE == in_off and in_off % 16 == 0 and arenas.out_ptr(k) % U.LINE == residue
        rc = lib.dxtlt_debug_pixels_auto_candidates_into_device(arenas.in_ptr(k), flat.size, B, arenas.out_ptr(k), stream)
        assert rc == OK, (jobs[k], lib.dxtlt_last_error())
    torch.cuda.synchronize()
    report = U.arena_differences(arenas.dst.cpu().numpy(), [(arenas.out_off[k], ref, jobs[k]) for k, (_f, ref) in enumerate(data)])
    assert not report, report
    assert torch.equal(arenas.src, arenas.src_before), "input written"


@gpu
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("P", U.CANDIDATE_COUNTS)
def test_single_kernel_at_every_tile_shape(lib, dev, B, P):
    run_single(lib, dev, [(P, B, 0, 0)])


@gpu
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("P", [4097, 12287])
def test_single_kernel_at_every_arena_residue(lib, dev, B, P):
    """in the calls candidate i starts i * len past a 256-byte boundary: every residue of a 16-byte line"""
    run_single(lib, dev, [(P, B, 0, r) for r in range(16)])


@gpu
@pytest.mark.parametrize("B", [3, 4])
def test_single_kernel_at_input_offsets_of_a_line(lib, dev, B):
    run_single(lib, dev, [(4097, B, off, (off // 16 + 5) % 16) for off in (0, 16, 48, 112)])


@gpu
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("P", LAST_LANE_COUNTS)
def test_single_kernel_at_every_valid_of_the_last_lane(lib, dev, B, P):
    run_single(lib, dev, [(P, B, 0, P % 16)])


@gpu
@pytest.mark.parametrize("B", [3, 4])
def test_single_kernel_where_a_plane_outgrows_a_window_bytes_and_totals(lib, dev, B):
    """32768 + 7 pixels: the byte check and the totals check on one shape -- the totals of dxtlt_transform_pixels_auto_device are the
    estimates of the very bytes the arena was held to"""
    import torch

    P = U.WINDOW + 7
    run_single(lib, dev, [(P, B, 0, 3)])
    flat, ref = single_input(P, B)
    x = torch.from_numpy(flat.copy()).to(dev)
    y = torch.empty_like(x)
    dec, lay = C.c_bool(), C.c_uint8(9)
    assert lib.dxtlt_transform_pixels_auto_device(x.data_ptr(), y.data_ptr(), flat.size, B, torch.cuda.current_stream().cuda_stream,
                                                  C.byref(dec), C.byref(lay)) == OK, lib.dxtlt_last_error()
    buf = (C.c_uint64 * 8)()
    assert lib.dxtlt_debug_pixels_auto_last_totals(buf, 8) == 6
    want = [R.estimate(ref[i * flat.size:(i + 1) * flat.size]) for i in range(5)] + [R.estimate(flat)]
    assert [int(v) for v in buf[:6]] == want
    assert (dec.value, lay.value) == R.CANDIDATES[R.pick(want)]
    torch.cuda.synchronize()


@gpu
def test_single_hook_refusals_write_nothing(lib, dev):
    import torch

    flat, ref = single_input(4097, 4)
    arenas = U.Arenas(dev, [flat], [0], [0], out_lengths=[ref.size])
    stream = torch.cuda.current_stream().cuda_stream
    hook = lib.dxtlt_debug_pixels_auto_candidates_into_device
    src, dst = arenas.in_ptr(0), arenas.out_ptr(0)
    assert hook(src, flat.size - 1, 4, dst, stream) == E_LENGTH             # not a multiple of pixel_bytes
    assert hook(src, flat.size - 4, 3, dst, stream) == E_LENGTH
    assert hook(src, flat.size, 5, dst, stream) == E_ARGUMENT
    assert hook(src, 0, 4, dst, stream) == E_ARGUMENT                       # an empty buffer
    assert hook(None, flat.size, 4, dst, stream) == E_ARGUMENT
    assert hook(src + 4, flat.size - 4, 4, dst, stream) == E_ARGUMENT       # off a 16-byte boundary: not the fused route's input
    assert hook(src, flat.size, 4, None, stream) == E_ARGUMENT
    torch.cuda.synchronize()
    assert U.arena_differences(arenas.dst.cpu().numpy(), []) == []
    assert torch.equal(arenas.src, arenas.src_before)


# ---- the batch kernel --------------------------------------------------------------------------------------------------------------------
class Batch:
    """the inputs of a case list on the device at their residues (and outputs that no candidate launch may touch), the items, the plan
    at the cap in force, and run(chunk): that chunk alone into a freshly filled arena of the call's size, held to the statement"""

    def __init__(self, lib, dev, name):
        self.lib, self.dev = lib, dev
        self.cases, self.flats, self.refs = batch_input(name)
        self.n = len(self.cases)
        self.arenas = U.Arenas(dev, self.flats, [c[5] for c in self.cases], [c[6] for c in self.cases])
        self.arr = U.make_auto_items(self.cases, self.arenas)
        self.replan()

    def replan(self):
        self.items, self.chunks = U.auto_plan(self.lib, self.arr, self.n)
        self.arena_bytes = max(ch.arena_bytes for ch in self.chunks)

    def fresh_arena(self):
        import torch

        t = torch.full((U.GUARD + self.arena_bytes + U.GUARD,), U.ARENA_FILL, dtype=torch.uint8, device=self.dev)
        assert t.data_ptr() % 256 == 0
        return t

    def placed(self, chunk):
        return [(U.GUARD + self.items[k].arena_offset, self.refs[k], (k,) + self.cases[k]) for k in range(self.n)
                if self.items[k].chunk == chunk and self.flats[k].size]

    def run(self, chunk):
        import torch

        arena = self.fresh_arena()
        rc = self.lib.dxtlt_debug_pixels_batch_candidates_device(self.arr, self.n, chunk, arena.data_ptr() + U.GUARD, self.arena_bytes,
                                                                 torch.cuda.current_stream().cuda_stream)
        assert rc == OK, (chunk, self.lib.dxtlt_last_error())
        host = arena.cpu().numpy()
        report = U.arena_differences(host, self.placed(chunk))
        assert not report, (chunk, report)
        assert all((a.decorrelate, a.layout) == (0xEE, 0xEE) for a in self.arr[:self.n])      # no result written
        self.arenas.check(written=())                                                         # no d_output, no input
        return host


@gpu
def test_mixed_batch_every_slice_and_every_padding_byte(lib, dev):
    b = Batch(lib, dev, "mixed")
    assert len(b.chunks) == 1 and b.chunks[0].candidate_launches == 2
    b.run(0)


@gpu
def test_forced_chunks_each_alone_into_a_fresh_arena(lib, dev):
    """under a cap: a chunk's items are exact and everything else -- the slices of the chunks that were not run, the padding, all that
    lies behind this chunk's arena_bytes -- keeps the fill"""
    b = Batch(lib, dev, "mixed")
    lib.dxtlt_debug_batch_auto_arena_cap(U.CANDIDATE_CHUNK_CAP)
    try:
        b.replan()
        assert len(b.chunks) >= 3
        for c, ch in enumerate(b.chunks):
            host = b.run(c)
            assert (host[U.GUARD + ch.arena_bytes:] == U.ARENA_FILL).all(), c
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)


@gpu
def test_wide_index_batch(lib, dev):
    b = Batch(lib, dev, "wide")
    assert len(b.chunks) == 1 and b.chunks[0].candidate_launches == 1
    b.run(0)


@gpu
def test_batch_slices_equal_the_single_kernel_item_by_item(lib, dev):
    import torch

    b = Batch(lib, dev, "mixed")
    batch_host = b.run(0)
    aligned = U.Arenas(dev, b.flats, [0] * b.n, [c[6] for c in b.cases])       # the single kernel reads from a 16-byte boundary
    arena = b.fresh_arena()
    stream = torch.cuda.current_stream().cuda_stream
    for k, flat in enumerate(b.flats):
        if flat.size:
            rc = lib.dxtlt_debug_pixels_auto_candidates_into_device(aligned.in_ptr(k), flat.size, b.cases[k][1],
                                                                    arena.data_ptr() + U.GUARD + b.items[k].arena_offset, stream)
            assert rc == OK, (k, lib.dxtlt_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(arena.cpu().numpy(), batch_host)
    aligned.check(written=())


@gpu
def test_the_python_layer_reaches_both_hooks(pkg, lib, dev):
    """dxt_lossless_transform_amd.pixels.debug_auto_candidates_into / debug_batch_candidates: the same arenas through the package"""
    import torch

    from dxt_lossless_transform_amd import pixels

    data = [single_input(4097, 4), single_input(12287, 3)]
    xs = [torch.from_numpy(flat.copy()).to(dev) for flat, _ref in data]
    ys = [torch.full_like(x, U.ARENA_FILL) for x in xs]
    for x, (flat, ref), B in zip(xs, data, (4, 3)):
        arena = torch.full((U.GUARD + ref.size + U.GUARD,), U.ARENA_FILL, dtype=torch.uint8, device=dev)
        pixels.debug_auto_candidates_into(x, arena[U.GUARD:U.GUARD + ref.size], B)
        torch.cuda.synchronize()
        assert not U.arena_differences(arena.cpu().numpy(), [(U.GUARD, ref, B)])
        with pytest.raises(pkg.OutputBufferTooSmall):
            pixels.debug_auto_candidates_into(x, arena[:ref.size - 1], B)
    arr = (U.AutoItem * 2)()
    for k, (x, y, B) in enumerate(zip(xs, ys, (4, 3))):
        arr[k].d_input, arr[k].d_output, arr[k].len, arr[k].pixel_bytes = x.data_ptr(), y.data_ptr(), x.numel(), B
    items, chunks = U.auto_plan(lib, arr, 2)
    size = chunks[0].arena_bytes
    arena = torch.full((U.GUARD + size + U.GUARD,), U.ARENA_FILL, dtype=torch.uint8, device=dev)
    pixels.debug_batch_candidates([(xs[0], ys[0], 4), (xs[1], ys[1], 3)], 0, arena[U.GUARD:U.GUARD + size])
    assert not U.arena_differences(arena.cpu().numpy(), [(U.GUARD + items[k].arena_offset, data[k][1], k) for k in range(2)])
    assert all(bool((y == U.ARENA_FILL).all()) for y in ys)
    with pytest.raises(pkg.DeviceError):
        pixels.debug_batch_candidates([(xs[0], ys[0], 4)], 1, arena[U.GUARD:U.GUARD + size])       # no such chunk
    assert not U.arena_differences(arena.cpu().numpy(), [(U.GUARD + items[k].arena_offset, data[k][1], k) for k in range(2)])


@gpu
def test_batch_hook_refusals_write_nothing(lib, dev):
    import torch

    b = Batch(lib, dev, "mixed")
    arena = b.fresh_arena()
    hook, at = lib.dxtlt_debug_pixels_batch_candidates_device, arena.data_ptr() + U.GUARD
    stream = torch.cuda.current_stream().cuda_stream
    assert hook(b.arr, b.n, 1, at, b.arena_bytes, stream) == E_ARGUMENT and b"chunk" in lib.dxtlt_last_error()
    assert hook(b.arr, 0, 0, at, b.arena_bytes, stream) == E_ARGUMENT                        # no items: no chunk
    assert hook(None, b.n, 0, at, b.arena_bytes, stream) == E_ARGUMENT
    assert hook(b.arr, b.n, 0, at, b.arena_bytes - 1, stream) == E_ARGUMENT and b"arena" in lib.dxtlt_last_error()
    assert hook(b.arr, b.n, 0, None, b.arena_bytes, stream) == E_ARGUMENT
    # what the call refuses, with its status
    saved = b.arr[3].d_output
    b.arr[3].d_output = b.arenas.in_ptr(0)
    assert hook(b.arr, b.n, 0, at, b.arena_bytes, stream) == E_ARGUMENT and b"overlaps" in lib.dxtlt_last_error()
    b.arr[3].d_output = saved
    b.arr[3].len -= 1
    assert hook(b.arr, b.n, 0, at, b.arena_bytes, stream) == E_LENGTH
    b.arr[3].len += 1
    # a capturing stream
    x = torch.arange(400, dtype=torch.uint8, device=dev)
    y = torch.zeros_like(x)
    assert lib.dxtlt_transform_pixels_device(x.data_ptr(), y.data_ptr(), 400, 4, False, 0, stream) == OK     # module load outside the capture
    torch.cuda.synchronize()
    y.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        rc = hook(b.arr, b.n, 0, at, b.arena_bytes, s)
        error = lib.dxtlt_last_error()
        marker = lib.dxtlt_transform_pixels_device(x.data_ptr(), y.data_ptr(), 400, 4, False, 0, s)          # capturable
    assert rc == E_ARGUMENT and b"capturable" in error and marker == OK
    graph.replay()                                                                                        # the capture is still alive
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    assert U.arena_differences(arena.cpu().numpy(), []) == []
    assert all((a.decorrelate, a.layout) == (0xEE, 0xEE) for a in b.arr[:b.n])
    b.arenas.check(written=())
