"""The candidate kernels of the BC1 - BC5 auto transforms -- auto_candidates_kernel<1|2|3, fast|all> and
auto_candidates_bc1_last_block<fast|all> (csrc/auto_kernels.hip), batch_auto_candidates_kernel<1..5, fast|all>
(csrc/batch_auto_kernels.hip), all of them candidate_lane of csrc/auto_candidate_lanes.h -- held to their statement BYTE FOR BYTE:
every section of an arena or slice is what tests/auto_candidates_ref.py cuts from the CPU transforms, and no other byte is written.
The calls show these bytes to nothing but the gram estimator, whose totals cannot see two windows changing places, a wrong byte
among unique grams or a write outside the arena (tests/test_auto_candidates_cases.py, no device needed); here two test hooks run
the kernels into memory of the test's own: dxtlt_debug_auto_candidates_into_device and dxtlt_debug_batch_auto_candidates_device
(include/dxtlt_estimator.h).

Every arena is device memory filled with 0xEE, 256 bytes of it at least in front of and behind every arena; K.differences is the
one comparison: every slice equal to the statement, every other byte still the fill.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import auto_candidates_ref as K
import batch_auto_util as BU
import estimator_ref as R
import pixels_gpu_common as G
import wide_common as W

pytestmark = pytest.mark.gpu

OK, E_LENGTH, E_ARGUMENT = K.OK, K.E_LENGTH, K.E_ARGUMENT
SOURCE_FILL = 0x11


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return K.load(pkg)


def current_stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


# ---- the single kernel -----------------------------------------------------------------------------------------------------------------
class SingleRun:
    """inputs in one device arena, arenas of the kernel in another (fill 0xEE, 256 bytes and more around each, pixels_gpu_common.Arena);
    launch() as often as wanted, then check(): one synchronise, one download, the one comparison"""

    def __init__(self, dev, jobs):
        """jobs: [(fmt, use_all, blocks, input bytes, statement, input offset 0..255, arena residue 0..255)]"""
        self.jobs = jobs
        a_in, a_out = G.Arena(), G.Arena()
        self.in_at = [a_in.place(j[5], j[3].size) for j in jobs]
        self.out_at = [a_out.place(j[6], j[4].size) for j in jobs]
        self.h_src = np.full(a_in.size(), SOURCE_FILL, dtype=np.uint8)
        for j, at in zip(jobs, self.in_at):
            self.h_src[at:at + j[3].size] = j[3]
        self.d_src = G.device_arena(dev, self.h_src)
        self.d_out = G.device_arena(dev, np.full(a_out.size(), K.FILL, dtype=np.uint8))

    def src(self, k):
        return self.d_src.data_ptr() + self.in_at[k]

    def dst(self, k):
        return self.d_out.data_ptr() + self.out_at[k]

    def launch(self, lib, k):
        fmt, use_all, _n, x, want = self.jobs[k][:5]
        assert self.src(k) % 256 == self.jobs[k][5] and self.dst(k) % 256 == self.jobs[k][6]
        rc = lib.dxtlt_debug_auto_candidates_into_device(fmt, use_all, self.src(k), x.size, self.dst(k), want.size, current_stream())
        assert rc == OK, (self.jobs[k][:3], self.jobs[k][5:], lib.dxtlt_last_error())

    def check(self, written=None):
        import torch

        torch.cuda.synchronize()
        placed = [(at, j[4], j[:3], j[:3] + j[5:]) for k, (j, at) in enumerate(zip(self.jobs, self.out_at)) if written is None or k in written]
        report = K.differences(self.d_out.cpu().numpy(), placed)
        assert not report, report
        assert np.array_equal(self.d_src.cpu().numpy(), self.h_src), "an input was written"


@pytest.mark.parametrize("fmt,use_all", K.SINGLE_GROUPS)
def test_single_kernel_every_count_offset_and_residue(lib, dev, oracle, fmt, use_all):
    """N in 1..66, around one and two workgroups, 4096 + 0..7 -- every N mod 8, so every residue mod 16 of a section start; odd BC1
    counts run the last-block kernel, N = 1 runs it alone -- inputs at 0, 16 and 80 bytes past a 256-byte boundary, arenas at residues
    0, 16, 48 and 112 of a 128-byte line"""
    jobs = [(fmt, use_all, n) + K.random_input(oracle, fmt, use_all, n) + (off, res) for n, off, res in K.single_jobs(fmt)]
    run = SingleRun(dev, jobs)
    for k in range(len(jobs)):
        run.launch(lib, k)
    run.check()


@pytest.mark.parametrize("fmt", [2, 1])
def test_every_colour_in_either_half_of_a_dword(lib, dev, oracle, fmt):
    """all four variants of 8 * 65 536 colour pairs: every 565 value in the low and in the high half of the dword decorrelate2 takes,
    against 0x0000, 0xFFFF, its complement and a permutation -- for BC1 in both colour dwords of a vector.  A carry between the packed
    halves shows in some variant."""
    x = K.every_colour_blocks(fmt)
    want = K.statement(oracle, fmt, True, x)
    run = SingleRun(dev, [(fmt, True, x.size // K.BLOCK[fmt], x, want, 0, 0)])
    run.launch(lib, 0)
    run.check()


def test_single_hook_refusals_write_nothing(lib, dev, oracle):
    x, want = K.random_input(oracle, 2, False, 66)
    y, want1 = K.random_input(oracle, 1, True, 33)
    run = SingleRun(dev, [(2, False, 66, x, want, 0, 0), (1, True, 33, y, want1, 16, 16)])
    hook, s = lib.dxtlt_debug_auto_candidates_into_device, current_stream()
    src, dst = run.src(0), run.dst(0)
    for fmt in (0, 4, 5, 6, -1):
        assert hook(fmt, False, src, x.size, dst, want.size, s) == E_ARGUMENT, fmt
    assert hook(2, False, src, x.size - 8, dst, want.size, s) == E_ARGUMENT           # half a block
    assert hook(1, True, run.src(1), y.size - 4, run.dst(1), want1.size, s) == E_ARGUMENT
    for off in (1, 4, 8):
        assert hook(2, False, src + off, x.size - 16, dst, want.size, s) == E_ARGUMENT, off
        assert hook(2, False, src, x.size - 16, dst + off, want.size - off, s) == E_ARGUMENT, off
    assert hook(2, False, src, x.size, dst, want.size - 1, s) == E_ARGUMENT and b"arena" in lib.dxtlt_last_error()
    assert hook(2, True, src, x.size, dst, want.size, s) == E_ARGUMENT                  # all modes need twice the colour sections
    assert hook(2, False, None, x.size, dst, want.size, s) == E_ARGUMENT
    assert hook(2, False, src, x.size, None, want.size, s) == E_ARGUMENT
    assert hook(2, False, None, 0, None, 0, s) == OK and hook(1, True, src, 0, dst, 0, s) == OK      # empty: nothing to do
    run.check(written=())
    run.launch(lib, 1)                                                                  # and the hook still works
    run.check(written=(1,))


# ---- the batched kernel ------------------------------------------------------------------------------------------------------------------
_BATCH_INPUTS = {}


def batch_inputs(oracle, cases):
    key = tuple(cases)
    if key not in _BATCH_INPUTS:
        _BATCH_INPUTS[key] = [K.random_input(oracle, fmt, use_all, n, seed=1 + k) for k, (fmt, use_all, n, _m) in enumerate(cases)]
    return _BATCH_INPUTS[key]


class Batch:
    """the inputs of a case list on the device at their misalignments, outputs that no candidate launch may touch, the items, the plan
    at the cap in force, and run(chunk): that chunk alone into a freshly filled arena of the call's size, held to the statement"""

    def __init__(self, lib, dev, oracle, cases):
        import torch

        self.lib, self.dev, self.cases, self.n = lib, dev, cases, len(cases)
        self.data = batch_inputs(oracle, cases)
        a_in, a_out = G.Arena(), G.Arena()
        self.in_at = [a_in.place(c[3], x.size) for c, (x, _w) in zip(cases, self.data)]
        out_at = [a_out.place(0, x.size) for x, _w in self.data]
        self.h_src = np.full(a_in.size(), SOURCE_FILL, dtype=np.uint8)
        for (x, _w), at in zip(self.data, self.in_at):
            self.h_src[at:at + x.size] = x
        self.d_src = G.device_arena(dev, self.h_src)
        self.d_out = torch.full((a_out.size(),), K.FILL, dtype=torch.uint8, device=dev)
        self.arr = BU.make_items([(c[0], self.d_src.data_ptr() + i if x.size else None, self.d_out.data_ptr() + o if x.size else None,
                                   x.size, c[1]) for c, (x, _w), i, o in zip(cases, self.data, self.in_at, out_at)])
        assert all(self.arr[k].d_input is None or self.arr[k].d_input % 16 == cases[k][3] for k in range(self.n))
        self.replan()

    def replan(self):
        self.items, self.chunks = K.auto_plan(self.lib, self.arr, self.n)
        self.arena_bytes = max(ch.arena_bytes for ch in self.chunks)

    def fresh_arena(self):
        import torch

        t = torch.full((K.GUARD + self.arena_bytes + K.GUARD,), K.FILL, dtype=torch.uint8, device=self.dev)
        assert t.data_ptr() % 256 == 0
        return t

    def placed(self, chunk):
        return [(K.GUARD + self.items[k].arena_offset, self.data[k][1], self.cases[k][:3], (k,) + self.cases[k]) for k in range(self.n)
                if self.items[k].chunk == chunk and self.data[k][0].size]

    def untouched(self):
        """no result field, no d_output, no input was written"""
        assert all((a.decorrelation_mode, a.split_alpha_endpoints, a.split_colour_endpoints) == (0xEE, 0xEE, 0xEE) for a in self.arr[:self.n])
        assert bool((self.d_out == K.FILL).all()), "a d_output was written"
        assert np.array_equal(self.d_src.cpu().numpy(), self.h_src), "an input was written"

    def run(self, chunk):
        arena = self.fresh_arena()
        rc = self.lib.dxtlt_debug_batch_auto_candidates_device(self.arr, self.n, chunk, arena.data_ptr() + K.GUARD, self.arena_bytes,
                                                               current_stream())
        assert rc == OK, (chunk, self.lib.dxtlt_last_error())
        host = arena.cpu().numpy()
        report = K.differences(host, self.placed(chunk))
        assert not report, (chunk, report)
        self.untouched()
        return host


def test_mixed_batch_every_slice_and_every_padding_byte(lib, dev, oracle):
    """41 items over all eight (format, use_all) launches, inputs at every misalignment 0..15 -- every launch with vector, dword and
    byte loads -- an empty item, the half lane alone, as the last lane of a workgroup and as lane 0 of a workgroup of its own"""
    b = Batch(lib, dev, oracle, K.cases_mixed())
    assert len(b.chunks) == 1 and b.chunks[0].candidate_launches == 8
    b.run(0)


def test_forced_chunks_each_alone_into_a_fresh_arena(lib, dev, oracle):
    """under a cap: a chunk's items are exact at offsets that restart with the chunk, and everything else -- the slices of the chunks
    that were not run, the padding, all that lies behind this chunk's arena_bytes -- keeps the fill"""
    b = Batch(lib, dev, oracle, K.cases_mixed())
    lib.dxtlt_debug_batch_auto_arena_cap(K.MIXED_CHUNK_CAP)
    try:
        b.replan()
        assert len(b.chunks) >= 3
        for c, ch in enumerate(b.chunks):
            assert b.items[ch.first_item].arena_offset == 0
            host = b.run(c)
            assert (host[K.GUARD + ch.arena_bytes:] == K.FILL).all(), c
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)


@pytest.mark.parametrize("count", [1, 2])
def test_batches_of_one_and_two_items(lib, dev, oracle, count):
    """no bisection step, and one"""
    b = Batch(lib, dev, oracle, K.cases_count(count))
    assert len(b.chunks) == 1 and b.chunks[0].candidate_launches == 1
    b.run(0)


def test_three_hundred_items_of_one_launch(lib, dev, oracle):
    """nine steps of bisection over first_wg, the half lane in every position"""
    b = Batch(lib, dev, oracle, K.cases_deep())
    assert len(b.chunks) == 1 and b.chunks[0].candidate_launches == 1
    b.run(0)


def test_first_middle_and_last_entry_own_several_workgroups(lib, dev, oracle):
    b = Batch(lib, dev, oracle, K.cases_owners())
    assert len(b.chunks) == 1 and b.chunks[0].candidate_launches == 1
    b.run(0)


def test_batch_slices_equal_the_single_kernel(lib, dev, oracle):
    """one item per BC1 - BC3 launch of the mixed batch: its slice is, byte for byte, the single hook's arena for the same input"""
    b = Batch(lib, dev, oracle, K.cases_mixed())
    host = b.run(0)
    picks = [next(k for k, c in enumerate(b.cases) if c[:2] == g and c[2] >= 4096) for g in K.SINGLE_GROUPS]
    run = SingleRun(dev, [b.cases[k][:3] + b.data[k] + (0, 0) for k in picks])
    for j in range(len(picks)):
        run.launch(lib, j)
    run.check()
    single = run.d_out.cpu().numpy()
    for j, k in enumerate(picks):
        size = b.data[k][1].size
        assert b.items[k].arena_bytes == size
        at = K.GUARD + b.items[k].arena_offset
        assert np.array_equal(host[at:at + size], single[run.out_at[j]:run.out_at[j] + size]), b.cases[k]


def test_batch_hook_refusals_write_nothing(lib, dev, oracle):
    import torch

    b = Batch(lib, dev, oracle, K.cases_mixed())
    arena = b.fresh_arena()
    hook, at, s = lib.dxtlt_debug_batch_auto_candidates_device, arena.data_ptr() + K.GUARD, current_stream()
    assert hook(b.arr, b.n, 1, at, b.arena_bytes, s) == E_ARGUMENT and b"chunk" in lib.dxtlt_last_error()
    assert hook(b.arr, 0, 0, at, b.arena_bytes, s) == E_ARGUMENT                         # no items: no chunk
    assert hook(None, b.n, 0, at, b.arena_bytes, s) == E_ARGUMENT
    assert hook(b.arr, b.n, 0, at, b.arena_bytes - 1, s) == E_ARGUMENT and b"arena" in lib.dxtlt_last_error()
    assert hook(b.arr, b.n, 0, None, b.arena_bytes, s) == E_ARGUMENT
    for off in (1, 4, 8):
        assert hook(b.arr, b.n, 0, at + off, b.arena_bytes, s) == E_ARGUMENT, off
    # what the call refuses, with its status
    saved = b.arr[3].d_output
    b.arr[3].d_output = b.arr[0].d_input
    assert hook(b.arr, b.n, 0, at, b.arena_bytes, s) == E_ARGUMENT and b"overlaps" in lib.dxtlt_last_error()
    b.arr[3].d_output = saved
    b.arr[3].len -= 1
    assert hook(b.arr, b.n, 0, at, b.arena_bytes, s) == E_LENGTH
    b.arr[3].len += 1
    b.arr[3].format = 6
    assert hook(b.arr, b.n, 0, at, b.arena_bytes, s) == E_ARGUMENT and b"format" in lib.dxtlt_last_error()
    b.arr[3].format = b.cases[3][0]
    # a capturing stream
    x = torch.arange(64, dtype=torch.uint8, device=dev)
    y = torch.zeros_like(x)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = hook(b.arr, b.n, 0, at, b.arena_bytes, current_stream())
        error = lib.dxtlt_last_error()
        y.copy_(x)
    assert rc == E_ARGUMENT and b"capturable" in error
    graph.replay()                                                                        # the capture is still alive
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    assert K.differences(arena.cpu().numpy(), []) == []
    b.untouched()
    b.run(0)                                                                              # and the hook still works


# ---- the hooks and the calls fill one layout ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,use_all", [(1, False), (2, True), (3, True), (4, False), (5, False)])
def test_the_calls_totals_are_the_estimates_of_the_statement(pkg, lib, dev, oracle, fmt, use_all):
    """dxtlt_transform_bcN_auto_device's totals == tests/estimator_ref.py over the sections the arenas above were held to, added up per
    candidate; for BC1 - BC3 the same input first goes through the hook (here through the Python layer) and the byte comparison"""
    import torch

    from dxt_lossless_transform_amd import estimator
    from oracle import oracle_auto

    name, n = K.FMT[fmt], 4097
    x = BU.auto_input(name, n, 3 if fmt <= 3 else 1, 5)
    want = K.statement(oracle, fmt, use_all, x)
    secs = K.sections(fmt, use_all, n)
    est = [R.estimate(want[off:off + length]) for _name, off, length, _per in secs]
    if fmt == 4:
        totals = est
    elif fmt == 5:
        totals = [est[0] + est[2], est[1] + est[3]]
    else:
        colour0 = 2 if fmt == 3 else 0
        totals = [est[colour0 + 2 * v + sc] + (est[sa] if fmt == 3 else 0) for v, sa, sc in oracle_auto.test_order(name, use_all)]
    assert len(set(totals)) >= 2
    d_x = torch.from_numpy(x).to(dev)
    if fmt <= 3:
        arena = torch.full((K.GUARD + want.size + K.GUARD,), K.FILL, dtype=torch.uint8, device=dev)
        estimator.debug_auto_candidates_into(name, d_x, arena[K.GUARD:K.GUARD + want.size], use_all)
        torch.cuda.synchronize()
        assert not K.differences(arena.cpu().numpy(), [(K.GUARD, want, (fmt, use_all, n), name)])
        assert estimator.auto_sections_bytes(name, x.size, use_all) == want.size
        with pytest.raises(pkg.OutputBufferTooSmall):
            estimator.debug_auto_candidates_into(name, d_x, arena[:want.size - 16], use_all)
    d_y = torch.empty_like(d_x)
    estimator.transform_auto(name, d_x, d_y, use_all)
    assert estimator.last_auto_totals() == totals
    torch.cuda.synchronize()
    assert torch.equal(d_x.cpu(), torch.from_numpy(x))


def test_the_python_layer_reaches_the_batch_hook(pkg, lib, dev, oracle):
    import torch

    from dxt_lossless_transform_amd import estimator

    cases = [(3, True, 257, 0), (4, False, 513, 0), (5, False, 66, 0)]
    data = [K.random_input(oracle, *c[:3]) for c in cases]
    xs = [torch.from_numpy(np.array(x)).to(dev) for x, _w in data]
    ys = [torch.full_like(x, K.FILL) for x in xs]
    items = [(K.FMT[c[0]], x, y, c[1]) for c, x, y in zip(cases, xs, ys)]
    arr = BU.make_items([(c[0], x.data_ptr(), y.data_ptr(), x.numel(), c[1]) for c, x, y in zip(cases, xs, ys)])
    plan, chunks = K.auto_plan(lib, arr, 3)
    size = chunks[0].arena_bytes
    arena = torch.full((K.GUARD + size + K.GUARD,), K.FILL, dtype=torch.uint8, device=dev)
    estimator.debug_batch_candidates(items, 0, arena[K.GUARD:K.GUARD + size])
    placed = [(K.GUARD + plan[k].arena_offset, data[k][1], cases[k][:3], cases[k]) for k in range(3)]
    assert not K.differences(arena.cpu().numpy(), placed)
    assert all(bool((y == K.FILL).all()) for y in ys)
    with pytest.raises(pkg.DeviceError):
        estimator.debug_batch_candidates(items, 1, arena[K.GUARD:K.GUARD + size])          # no such chunk
    with pytest.raises(pkg.DeviceError):
        estimator.debug_batch_candidates(items, 0, arena[K.GUARD:K.GUARD + size - 16])     # a short arena
    assert not K.differences(arena.cpu().numpy(), placed)


# ---- the second grid row -------------------------------------------------------------------------------------------------------------------
WIDE_N = W.LANES                      # BC2 blocks = vectors: 2^20 + 4 workgroups, four of them in the second grid row
WIDE_SMALL = (66, 257)                # the two items in front of the wide one in the batch


class WideArena(W.Arena):
    """wide_common.Arena at the size these two cases need, and its skip rule: less free memory than the need plus 8 GiB"""

    def __init__(self, dev, nbytes):
        import torch

        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(dev)
        if free < nbytes + W.SPARE:
            pytest.skip(f"needs {nbytes / 2**30:.1f} GiB plus 8 GiB, {free >> 30} GiB were free")
        super().__init__(dev, nbytes)
        self.free = free


@pytest.fixture(scope="module")
def wide(dev, oracle):
    """one arena, the BC2 input of 2^28 + 845 pattern blocks (4 GiB) and what every section of its slice must hold, per pattern block"""
    import torch

    n = WIDE_N
    assert 16 * n > 1 << 32 and n > 256 * (1 << 20)
    a = WideArena(dev, 3 * 16 * n + (64 << 20))          # input, arena, and the d_output of the batched case
    pat = W.bcn_pattern("bc2")
    src = W.tiled(pat, n, a)
    want = K.statement(oracle, 2, False, np.ascontiguousarray(pat).reshape(-1))
    expected = []                                         # per section: [(offset in the slice / N, (P, rec) records)]
    for name, off, length, _per in K.sections(2, False, W.P):
        part = want[off:off + length]
        if "split" in name:                               # all c0, then all c1: two arrays of 2-byte records
            expected += [(name + ", c0", off // W.P, part[:2 * W.P].reshape(W.P, 2)), (name + ", c1", off // W.P + 2, part[2 * W.P:].reshape(W.P, 2))]
        else:
            expected.append((name, off // W.P, part.reshape(W.P, 4)))
    expected = [(name, per_block, torch.from_numpy(np.array(rec)).to(dev)) for name, per_block, rec in expected]
    yield a, pat, src, expected
    a.buf = None
    torch.cuda.empty_cache()


def wide_check(a, pat, src, expected, slice_view, n, what):
    import torch

    for name, per_block, rec in expected:
        at = per_block * n
        W.check_records(slice_view[at:at + rec.shape[1] * n], rec, n, f"{what}: section '{name}'")
    W.check_records(src, torch.from_numpy(np.array(pat)).to(src.device), n, f"{what}: the input")


def count_not(t, fill):
    return sum(int((t[lo:lo + W.CHUNK] != fill).sum()) for lo in range(0, t.numel(), W.CHUNK))


def test_single_kernel_in_the_second_grid_row(lib, wide):
    a, pat, src, expected = wide
    n, size = WIDE_N, 16 * WIDE_N
    a.used = src.numel()
    whole = a.take(K.GUARD + size + K.GUARD)
    whole.fill_(K.FILL)
    arena = whole[K.GUARD:K.GUARD + size]
    assert src.data_ptr() % 16 == 0 and arena.data_ptr() % 16 == 0 and size == K.slice_bytes(2, False, n)
    rc = lib.dxtlt_debug_auto_candidates_into_device(2, False, src.data_ptr(), 16 * n, arena.data_ptr(), size, current_stream())
    assert rc == OK, lib.dxtlt_last_error()
    wide_check(a, pat, src, expected, arena, n, "single kernel")
    assert count_not(whole[:K.GUARD], K.FILL) == 0 and count_not(whole[K.GUARD + size:], K.FILL) == 0, "guard bytes were written"


def test_batched_kernel_in_the_second_grid_row(lib, dev, oracle, wide):
    """the same item behind two small ones in ONE launch (the cap lifted, or it would be a chunk of its own): first_wg = 2, its lanes
    reach six workgroups into the second row"""
    import torch

    a, pat, src, expected = wide
    n = WIDE_N
    small = [K.random_input(oracle, 2, False, m) for m in WIDE_SMALL]
    xs = [torch.from_numpy(np.array(x)).to(dev) for x, _w in small]
    ys = [torch.full_like(x, K.FILL) for x in xs]
    a.used = src.numel()
    d_out = a.take(16 * n)                                 # never written, but the plan wants an output that overlaps nothing
    d_out.fill_(K.FILL)
    arr = BU.make_items([(2, x.data_ptr(), y.data_ptr(), x.numel(), False) for x, y in zip(xs, ys)] + [(2, src.data_ptr(), d_out.data_ptr(), 16 * n, False)])
    lib.dxtlt_debug_batch_auto_arena_cap(1 << 40)
    try:
        items, chunks = K.auto_plan(lib, arr, 3)
        assert len(chunks) == 1 and chunks[0].candidate_launches == 1 and items[2].arena_offset == 16 * sum(WIDE_SMALL)
        size = chunks[0].arena_bytes
        whole = a.take(K.GUARD + size + K.GUARD)
        whole.fill_(K.FILL)
        rc = lib.dxtlt_debug_batch_auto_candidates_device(arr, 3, 0, whole.data_ptr() + K.GUARD, size, current_stream())
        assert rc == OK, lib.dxtlt_last_error()
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)
    at = K.GUARD + items[2].arena_offset
    wide_check(a, pat, src, expected, whole[at:at + 16 * n], n, "batched kernel")
    head = whole[:at].cpu().numpy()                        # the guard in front and the two small slices
    placed = [(K.GUARD + items[k].arena_offset, small[k][1], (2, False, WIDE_SMALL[k]), k) for k in range(2)]
    assert not K.differences(head, placed)
    assert at + 16 * n == K.GUARD + size and count_not(whole[K.GUARD + size:], K.FILL) == 0, "guard bytes were written"
    assert all(bool((y == K.FILL).all()) for y in ys) and count_not(d_out, K.FILL) == 0, "a d_output was written"
