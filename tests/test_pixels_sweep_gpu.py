"""The pixel kernels (csrc/pixel_kernels.hip) swept on the device, byte for byte against tests/pixels_ref.py: every residue 0..127
of every plane base and of the interleaved pointer, every tail length at every wave and tile boundary, every byte pair in every
slot of a lane through subtract-green, the delta and the scan, every range call on its own, a seeded fuzz over the combinations,
and the `_device` calls on a side stream, replayed from a captured graph and on two streams at once.

Every test that runs many launches puts them into one arena (tests/pixels_gpu_common.py: run_jobs): each output between 256 bytes
of 0xA5, all launches issued, one synchronise, one download; every output equals the reference, every guard byte and every
source byte is unchanged.  Expected bytes are computed once per (B, settings, P) and do not depend on a residue.  The three case
lists whose completeness matters -- plane residues, subtract-green pairs, delta pairs -- each have a proof beside them that runs
without a device and asserts an exact count."""
import numpy as np
import pytest

import pixels_ref as R
from pixels_gpu_common import FILL, OK, Job, both_directions, case_jobs, draw_case, run_jobs

SEG = R.SEGMENT
LAYOUT_ID = {R.INTERLEAVED: "interleaved", R.PLANAR: "planar", R.PLANAR_DELTA: "delta"}
per_setting = pytest.mark.parametrize("decorrelate,layout", R.SETTINGS,
                                      ids=lambda v: ("green" if v else "plain") if isinstance(v, bool) else LAYOUT_ID[v])
per_B = pytest.mark.parametrize("B", [3, 4])


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    d = torch.device("cuda:0")
    torch.zeros(1, dtype=torch.uint8, device=d)
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def lib(pkg):
    import ctypes as C

    return R.declare(C.CDLL(pkg._lib.lib_path()))


# ---- expected bytes: once per (B, settings, P) -----------------------------------------------------------------------------------
_POOL, _STATEMENTS = {}, {}
POOL_PIXELS = 5 * SEG + 77 + 64


def statement(B, decorrelate, layout, P):
    """(pixels, their transform by the CPU statement) of a buffer of P pixels, read-only; the pixels are a window of one random pool
    per B, at an offset that changes with P"""
    key = (B, decorrelate, layout, P)
    if key not in _STATEMENTS:
        assert P + 64 <= POOL_PIXELS
        if B not in _POOL:
            _POOL[B] = np.random.default_rng(0x9E1 + B).integers(0, 256, POOL_PIXELS * B, dtype=np.uint8)
        if (B, P) not in _STATEMENTS:
            x = _POOL[B][(P % 64) * B:(P % 64 + P) * B].copy()
            x.setflags(write=False)
            _STATEMENTS[(B, P)] = x
        x = _STATEMENTS[(B, P)]
        want = np.ascontiguousarray(R.forward(x, B, decorrelate, layout))
        want.setflags(write=False)
        _STATEMENTS[key] = (x, want)
    return _STATEMENTS[key]


def whole_buffer_jobs(B, decorrelate, layout, cases):
    """cases: [(P, transformed-side residue, interleaved-side residue)]; both directions of each"""
    jobs = []
    for P, t, i in cases:
        x, want = statement(B, decorrelate, layout, P)
        jobs += both_directions(x, want, B, decorrelate, layout, t, i)
    return jobs


# ---- a. every residue, both sides ---------------------------------------------------------------------------------------------------
P_RES = 2 * SEG + 80                                  # a multiple of 16: every plane at the pointer's residue, residue 0 the fast form
I_CYCLE = (0, 1, 3, 4, 8, 12, 15, 16, 64)


def residue_lists():
    """(P, transformed-side residue, interleaved-side residue), three lists: the transformed pointer at every residue; both pointers
    aligned and P + q, which puts plane c at c q mod 128; the interleaved pointer at every residue against transformed residues 0, 1"""
    return ([(P_RES, r, I_CYCLE[r % len(I_CYCLE)]) for r in range(128)],
            [(P_RES + q, 0, 0) for q in range(128)],
            [(P_RES + 7, t, i) for t in (0, 1) for i in range(128)])


def residue_cases():
    """the three lists in one, each case once: (P_RES, 0, 0), the fast form, heads the first two, and (P_RES + 7, 0, 0) is in the last two"""
    return list(dict.fromkeys(c for part in residue_lists() for c in part))


def plane_residues(cases, B):
    """the set of (plane, residue mod 128 of its first byte) a case list reaches"""
    return {(c, (t + c * P) % 128) for P, t, _ in cases for c in range(B)}


@per_B
def test_residue_list_reaches_every_residue_of_every_plane(B):
    """No device.  From the list alone: every plane index starts on every residue 0..127, the interleaved pointer takes every
    residue, and the fast form (both pointers and P multiples of 16) is among the cases.  First the proof shows it can fail: the
    second list on its own never moves plane 0, and the first list thinned to even residues reaches half of them."""
    first, second, third = residue_lists()
    cases = residue_cases()
    assert (len(first), len(second), len(third)) == (128, 128, 256) and len(cases) == 510 and set(cases) == set(first + second + third)
    assert {r for c, r in plane_residues(second, B) if c == 0} == {0}
    assert {r for c, r in plane_residues(second, B) if c == 1} == set(range(128))
    thinned = [c for c in first if c[1] % 2 == 0]
    assert len(plane_residues(thinned, B)) == B * 64
    # the list itself
    reached = plane_residues(cases, B)
    assert len(reached) == B * 128 and reached == {(c, r) for c in range(B) for r in range(128)}
    assert plane_residues(first, B) == reached                     # the pointer sweep alone reaches them, P_RES being a multiple of 16
    for t in (0, 1):
        assert sorted(i for _, tt, i in third if tt == t) == list(range(128))
    assert {i for _, _, i in first} == set(I_CYCLE)
    assert sum(1 for P, t, i in cases if P % 16 == 0 and t % 16 == 0 and i % 16 == 0) >= 1
    assert (P_RES, 0, 0) in cases and P_RES % 16 == 0 and P_RES > 2 * SEG and P_RES % SEG >= 16


@pytest.mark.gpu
@per_setting
@per_B
def test_every_residue_of_both_pointers(lib, dev, B, decorrelate, layout):
    """two full tiles and a tail of 80 .. 207 pixels, forward and inverse, at the 510 (P, residue, residue) of residue_cases()"""
    run_jobs(lib, dev, whole_buffer_jobs(B, decorrelate, layout, residue_cases()))


# ---- b. every tail -------------------------------------------------------------------------------------------------------------------
def tail_counts():
    out = set(range(0, 289)) | set(range(SEG, SEG + 289))
    for c in (1024, 2048, 3072, 4096, 8192):                      # the wave boundaries of a tile, one tile, two tiles
        out |= set(range(c - 17, c + 18))
    return sorted(out)


def test_tail_counts_are_the_735():
    counts = tail_counts()
    assert len(counts) == 735 and counts[0] == 0 and counts[-1] == 8192 + 17
    for boundary in (1024, 2048, 3072):                            # valid = 1..15 in the lane behind a wave boundary, first and second tile
        assert {boundary + v for v in range(1, 16)} <= set(counts)
        assert {SEG + v for v in range(1, 16)} <= set(counts)
    assert {n * B % 16 for n in counts for B in (3, 4)} == set(range(16))     # every count of single bytes in stage_in / stage_out


@pytest.mark.gpu
@per_setting
@per_B
def test_every_tail(lib, dev, B, decorrelate, layout):
    """whole buffers of 735 pixel counts, interleaved side aligned, transformed side at residue 1: no access aligned by accident"""
    run_jobs(lib, dev, whole_buffer_jobs(B, decorrelate, layout, [(P, 1, 0) for P in tail_counts()]))


# ---- c. every byte pair through the kernels ---------------------------------------------------------------------------------------------
PAIR_PIXELS = 16 * 65536


def green_pair_pixels(B):
    """pixel i, j = i // 65536, holds pair p = (i + j) mod 65536: G = p >> 8, byte 0 = p & 255, byte 2 = (p & 255) ^ 0xA5"""
    i = np.arange(PAIR_PIXELS, dtype=np.int64)
    p = (i + i // 65536) % 65536
    px = np.zeros((PAIR_PIXELS, B), dtype=np.uint8)
    px[:, 1], px[:, 0], px[:, 2] = p >> 8, p & 255, (p & 255) ^ 0xA5
    if B == 4:
        px[:, 3] = (13 * i) % 256
    return px


@per_B
def test_green_pair_pixels_hold_every_pair_in_every_slot(B):
    """No device.  From the array: every (x, g) at every lane slot i mod 16, for byte 0 and for byte 2 -- 16 * 65 536 each, none
    missing; the same count on the first 15 of the 16 blocks is short, so the count can tell."""
    px = green_pair_pixels(B)
    slot = np.arange(PAIR_PIXELS) % 16
    for byte in (0, 2):
        key = (px[:, byte].astype(np.int64) * 256 + px[:, 1]) * 16 + slot
        seen = np.zeros(16 * 65536, dtype=bool)
        seen[key[:15 * 65536]] = True
        assert int(seen.sum()) == 15 * 65536
        seen[key] = True
        assert int(seen.sum()) == 16 * 65536 and int((~seen).sum()) == 0


_GREEN = {}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=lambda l: LAYOUT_ID[l])
@per_B
def test_subtract_green_at_every_byte_pair(lib, dev, B, layout):
    if B not in _GREEN:
        _GREEN[B] = green_pair_pixels(B).reshape(-1)
    x = _GREEN[B]
    run_jobs(lib, dev, both_directions(x, R.forward(x, B, True, layout), B, True, layout, 0, 0, ("green pairs",)))


def pair_sequence():
    """a, b for all a, b in 0..255: 131 072 bytes"""
    return np.stack([np.repeat(np.arange(256), 256), np.tile(np.arange(256), 256)], axis=1).reshape(-1).astype(np.uint8)


DELTA_SHIFTS = 17
DELTA_FILLER = 0x3C


def delta_planes(B, k):
    """(B, 131 072 + k): k filler bytes, then the sequence; plane c is that xor 0x55 c, so that the lane totals the inverse packs
    into one dword differ between the planes"""
    base = np.concatenate([np.full(k, DELTA_FILLER, dtype=np.uint8), pair_sequence()])
    return np.stack([base ^ np.uint8((0x55 * c) & 0xFF) for c in range(B)])


def delta_pixels(B, k, decorrelate):
    """pixels whose planes -- after subtract-green, when it is on -- are delta_planes(B, k)"""
    px = np.ascontiguousarray(delta_planes(B, k).T)
    if decorrelate:
        px[:, 0] += px[:, 1]
        px[:, 2] += px[:, 1]
    return px.reshape(-1)


def pairs_seen(planes, seen):
    """marks (byte in front, byte, slot of the byte in its lane's vector) for every byte that has one in front in its segment"""
    for c in range(planes.shape[0]):
        p = planes[c].astype(np.int64)
        i = np.arange(1, p.size)
        i = i[i % SEG != 0]
        seen[c, (p[i - 1] * 256 + p[i]) * 16 + i % 16] = True


@pytest.mark.parametrize("decorrelate", [False, True])
@per_B
def test_delta_pixels_hold_every_pair_in_every_slot(B, decorrelate):
    """No device.  From the pixels, through the planes the kernel takes differences of: every (previous byte, byte) in every slot of
    a lane's sixteen, in every plane -- 16 * 65 536 each.  Sixteen shifts leave exactly one uncovered (it falls on a segment's
    first byte, which has no byte in front); the seventeenth covers it."""
    seen = np.zeros((B, 16 * 65536), dtype=bool)
    for k in range(DELTA_SHIFTS):
        if k == 16:
            assert [int(n) for n in (~seen).sum(axis=1)] == [1] * B
        planes = R.forward(delta_pixels(B, k, decorrelate), B, decorrelate, R.PLANAR).reshape(B, -1)
        assert np.array_equal(planes, delta_planes(B, k))
        pairs_seen(planes, seen)
    assert [int(n) for n in seen.sum(axis=1)] == [16 * 65536] * B and int((~seen).sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("decorrelate", [False, True], ids=["plain", "green"])
@per_B
def test_delta_and_scan_at_every_byte_pair(lib, dev, B, decorrelate):
    """forward of the 17 buffers (the delta; with subtract-green the kernel's own decorrelation of the byte in front) and inverse
    of the reference's forward (the scan and the carries between lanes and waves)"""
    jobs = []
    for k in range(DELTA_SHIFTS):
        x = delta_pixels(B, k, decorrelate)
        jobs += both_directions(x, R.forward(x, B, decorrelate, R.PLANAR_DELTA), B, decorrelate, R.PLANAR_DELTA, 0, 0, ("delta pairs", k))
    run_jobs(lib, dev, jobs)


# ---- d. one range call at a time ----------------------------------------------------------------------------------------------------------
RANGE_TOTAL = 5 * SEG + 77
RANGE_PIECES = [(0, SEG), (SEG, 2 * SEG), (3 * SEG, RANGE_TOTAL - 3 * SEG), (SEG, 5000), (2 * SEG, 1), (0, RANGE_TOTAL)]
RANGE_PARTITION = [(3 * SEG, RANGE_TOTAL - 3 * SEG), (0, SEG), (SEG, 2 * SEG)]        # shuffled order
RANGE_RESIDUES = (3, 1)                                                                # (transformed side, interleaved side)


def range_image(whole, B, layout, inverse, pieces):
    """the output of the given range calls alone: the reference's bytes of the whole buffer where a piece owns them, FILL elsewhere"""
    image = np.full(RANGE_TOTAL * B, FILL, dtype=np.uint8)
    for first, num in pieces:
        if inverse or layout == R.INTERLEAVED:
            image[first * B:(first + num) * B] = whole[first * B:(first + num) * B]
        else:
            for c in range(B):
                image[c * RANGE_TOTAL + first:c * RANGE_TOTAL + first + num] = whole[c * RANGE_TOTAL + first:c * RANGE_TOTAL + first + num]
    return image


def test_range_pieces_are_what_they_claim():
    assert sorted(RANGE_PARTITION) == sorted(RANGE_PIECES[:3]) and RANGE_PARTITION != sorted(RANGE_PARTITION)
    at = 0
    for first, num in sorted(RANGE_PARTITION):
        assert first == at
        at += num
    assert at == RANGE_TOTAL
    assert all(first % SEG == 0 and first + num <= RANGE_TOTAL for first, num in RANGE_PIECES)
    first, num = RANGE_PIECES[3]
    assert (first + num) % SEG not in (0, RANGE_TOTAL % SEG) and first + num < RANGE_TOTAL     # ends inside a segment, buffer goes on
    assert (first + num) % 16 != 0 and num * 3 % 16 != 0


@pytest.mark.gpu
@per_setting
@per_B
def test_every_range_call_alone_and_a_partition(lib, dev, B, decorrelate, layout):
    """Each piece into an output of its own: inside the whole output exactly the piece's bytes are the reference's, every other
    byte is still 0xA5 -- so a piece that reaches into a neighbour's bytes shows, which a composed buffer hides.  Then the three
    pieces of a partition, out of order, into one output: the whole.  Both pointers misaligned."""
    x, want = statement(B, decorrelate, layout, RANGE_TOTAL)
    t, i = RANGE_RESIDUES
    jobs = []
    for inverse, src, whole in ((False, x, want), (True, want, x)):
        for pieces in [[p] for p in RANGE_PIECES] + [RANGE_PARTITION]:
            jobs.append(Job(inverse, B, decorrelate, layout, RANGE_TOTAL, pieces, src, t, i, range_image(whole, B, layout, inverse, pieces),
                            ("inverse" if inverse else "forward", "ranges", pieces, B, decorrelate, layout, t, i)))
        assert np.array_equal(jobs[-1].want, whole)
    run_jobs(lib, dev, jobs)


# ---- e. combination fuzz --------------------------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_CASES, FUZZ_ARENA = 0xF0891, 1500, 250


def fuzz_cases():
    rng = np.random.default_rng(FUZZ_SEED)
    return [draw_case(rng) for _ in range(FUZZ_CASES)]


def test_fuzz_draw_reaches_every_axis():
    """No device: what the 1500 draws contain, so that a change of the draw which empties an axis is noticed"""
    cases = fuzz_cases()
    assert len(cases) == FUZZ_CASES
    assert {(c.B, c.decorrelate, c.layout) for c in cases} == {(B, d, l) for B in (3, 4) for d, l in R.SETTINGS}
    assert {c.count_kind for c in cases} == {"tiny", "segments +- 17", "any", "vectors +- a few"}
    assert {c.data_kind for c in cases} == {"uniform", "walk", "constant", "alternating"}
    for side in ("in_off", "out_off"):
        offs = [getattr(c, side) for c in cases]
        assert offs.count(0) > FUZZ_CASES // 2 and len(set(offs)) > 100 and max(offs) <= 127
    ranged = [c for c in cases if c.cut]
    assert len(ranged) > 100 and all(c.cut % SEG == 0 and 0 < c.cut < c.P for c in ranged)
    assert {(c.B, c.decorrelate, c.layout) for c in ranged} == {(B, d, l) for B in (3, 4) for d, l in R.SETTINGS}
    assert max(c.P for c in cases) <= 70_000 and min(c.P for c in cases) == 0


@pytest.mark.gpu
def test_random_combinations(lib, dev):
    """1500 seeded cases, none left out, 250 to an arena: forward == reference, inverse of the reference == input, guards and
    sources untouched.  A failure names the case: (direction, index, B, decorrelate, layout, count kind, P, interleaved-side offset,
    transformed-side offset, cut, data kind, data seed); `python tools/fuzz_gpu.py --pixels` draws from the same function."""
    cases = fuzz_cases()
    for at in range(0, FUZZ_CASES, FUZZ_ARENA):
        jobs = []
        for index in range(at, min(at + FUZZ_ARENA, FUZZ_CASES)):
            jobs += case_jobs(cases[index], index)
        run_jobs(lib, dev, jobs)


# ---- f. graph capture and side streams ------------------------------------------------------------------------------------------------------
GRAPH_P = 2 * SEG + 77
GRAPH_SETTINGS = ((True, R.PLANAR_DELTA), (False, R.PLANAR))


@pytest.mark.gpu
def test_device_calls_replay_from_a_graph_captured_on_a_side_stream(lib, dev):
    """The `_device` calls only enqueue: warmed up and then captured on ONE side stream (a chain, no parallel branches) -- forward and
    inverse of two settings for both B, and one forward as two range calls --, then replayed once over fresh input with the outputs
    zeroed: only the replay can have produced the reference's bytes."""
    import torch

    def fresh(B, seed):
        return np.random.default_rng(seed).integers(0, 256, GRAPH_P * B, dtype=np.uint8)

    bufs = []           # (B, decorrelate, layout, ranged, x, y, z)
    for B in (3, 4):
        for decorrelate, layout in GRAPH_SETTINGS:
            x = torch.from_numpy(fresh(B, 10 + B)).to(dev)
            bufs.append((B, decorrelate, layout, False, x, torch.zeros_like(x), torch.zeros_like(x)))
    x = torch.from_numpy(fresh(4, 14)).to(dev)
    bufs.append((4, True, R.PLANAR_DELTA, True, x, torch.zeros_like(x), torch.zeros_like(x)))

    def work(stream):
        for B, decorrelate, layout, ranged, x, y, z in bufs:
            if ranged:
                for first, num in ((SEG, GRAPH_P - SEG), (0, SEG)):
                    assert lib.dxtlt_transform_pixels_range_device(B, False, x.data_ptr() + first * B, y.data_ptr(), GRAPH_P, first, num,
                                                                   decorrelate, layout, stream) == OK
            else:
                assert lib.dxtlt_transform_pixels_device(x.data_ptr(), y.data_ptr(), x.numel(), B, decorrelate, layout, stream) == OK
            assert lib.dxtlt_untransform_pixels_device(y.data_ptr(), z.data_ptr(), x.numel(), B, decorrelate, layout, stream) == OK

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        work(side.cuda_stream)                      # warm-up outside capture (module load, first launch)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    for B, decorrelate, layout, _, x, y, z in bufs:
        assert np.array_equal(y.cpu().numpy(), R.forward(x.cpu().numpy(), B, decorrelate, layout)) and torch.equal(z, x)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        work(torch.cuda.current_stream(dev).cuda_stream)
    inputs = []
    for k, (B, _, _, _, x, y, z) in enumerate(bufs):
        inputs.append(fresh(B, 100 + k))
        x.copy_(torch.from_numpy(inputs[-1]))
        y.zero_()
        z.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    for new, (B, decorrelate, layout, ranged, x, y, z) in zip(inputs, bufs):
        assert np.array_equal(x.cpu().numpy(), new)
        assert np.array_equal(y.cpu().numpy(), R.forward(new, B, decorrelate, layout)), ("forward", B, decorrelate, layout, ranged)
        assert np.array_equal(z.cpu().numpy(), new), ("inverse", B, decorrelate, layout, ranged)


@pytest.mark.gpu
def test_two_calls_on_two_streams_without_a_synchronise_between(lib, dev):
    """a forward call on one torch stream and an inverse call on another, issued back to back; each 64 tiles and a tail, long enough
    to be in flight together"""
    import torch

    P = 64 * SEG + 77
    x4 = np.random.default_rng(41).integers(0, 256, P * 4, dtype=np.uint8)
    x3 = np.random.default_rng(31).integers(0, 256, P * 3, dtype=np.uint8)
    t3 = R.forward(x3, 3, False, R.PLANAR)
    d_x4, d_t3 = torch.from_numpy(x4).to(dev), torch.from_numpy(np.ascontiguousarray(t3)).to(dev)
    d_y4, d_z3 = torch.zeros_like(d_x4), torch.zeros_like(d_t3)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    assert s1.cuda_stream != s2.cuda_stream
    s1.wait_stream(torch.cuda.current_stream(dev))
    s2.wait_stream(torch.cuda.current_stream(dev))
    assert lib.dxtlt_transform_pixels_device(d_x4.data_ptr(), d_y4.data_ptr(), x4.size, 4, True, R.PLANAR_DELTA, s1.cuda_stream) == OK
    assert lib.dxtlt_untransform_pixels_device(d_t3.data_ptr(), d_z3.data_ptr(), x3.size, 3, False, R.PLANAR, s2.cuda_stream) == OK
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_y4.cpu().numpy(), R.forward(x4, 4, True, R.PLANAR_DELTA))
    assert np.array_equal(d_z3.cpu().numpy(), x3)
    assert np.array_equal(d_x4.cpu().numpy(), x4) and np.array_equal(d_t3.cpu().numpy(), t3)
