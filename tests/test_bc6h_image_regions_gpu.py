"""Several images of one BC6H buffer on the MI355X (include/dxtlt_bc6h_image.h): the fused region call, the block-array call, the
host call, the Python wrappers and a HIP graph.  Every image is compared byte for byte with the numpy statement of
tests/bc6h_decode_ref.py AND with the bytes the single-image call writes for that region alone.  All images of a call live in one
arena prefilled with 0xA5: the guard bytes around and between them, the pitch padding and the pixels a clipped block does not
have must still be 0xA5 afterwards, and the source is unchanged.  Transformed buffers come from dxtlt_transform_bc6h.  The largest
buffer is 5463 blocks."""
import numpy as np
import pytest

import bc6h_decode_ref as ref
from bc6h_image_regions_common import (BPP, CHAIN_256, GRANULE, OK, PER_LAUNCH, THREE_FACES, TOTAL_256, TOTAL_THREE, TOTAL_TWO, TWO_FACES,
                                       blocks_of, groups_of, load, region_array, region_end)

pytestmark = pytest.mark.gpu

GUARD = 256
TOTALS = (1, 37, 1023, 1024, 1025, 2391, 5463)
KINDS = {"balanced": ref.mode_balanced_blocks, "wave_uniform": ref.wave_uniform_blocks, "interleaved": ref.interleaved_class_blocks}


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


_cache = {}


def reference_of(lib, key, make):
    """(blocks (total, 16), their pixels (total, 16, 4) uint16, the transformed buffer) of a whole array, computed once and shared"""
    if key not in _cache:
        x = make()
        t = np.zeros(x.size, dtype=np.uint8)
        assert lib.dxtlt_transform_bc6h(x.ctypes.data, t.ctypes.data, x.size) == OK
        px = ref.decode_blocks(x)
        for a in (x, t, px):
            a.setflags(write=False)
        _cache[key] = (x, px, t)
    return _cache[key]


def reference(lib, kind, total, seed=0):
    return reference_of(lib, (kind, total, seed), lambda: KINDS[kind](total, 500 + seed))


def expected_buffer(px, region, pitch):
    """the pitch * height bytes of an output prefilled with 0xA5 that received the region's image"""
    first, width, height = region
    out = np.full(pitch * height, 0xA5, dtype=np.uint8)
    if width and height:
        out.reshape(height, pitch)[:, :BPP * width] = ref.image_bytes(px[first:region_end(region)], width, height)
    return out


class Arena:
    """One device buffer of 0xA5 that holds payloads of `sizes[i]` bytes, payload i at `offs[i]` bytes behind a 256-byte aligned
    address, at least GUARD bytes of 0xA5 in front of, between and behind them"""

    def __init__(self, dev, sizes, offs=None, data=None):
        import torch

        offs = [0] * len(sizes) if offs is None else offs
        self.at, end = [], 0
        for n, off in zip(sizes, offs):
            start = (end + GUARD + 255) // 256 * 256 + off
            self.at.append(start)
            end = start + n
        self.sizes = list(sizes)
        self.base = torch.full((end + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert self.base.data_ptr() % 256 == 0
        if data is not None:
            for start, d in zip(self.at, data):
                d = np.ascontiguousarray(d).reshape(-1)
                self.base[start:start + d.size].copy_(torch.from_numpy(d.copy()).to(dev))
        self.ptrs = [self.base.data_ptr() + start for start in self.at]

    def view(self, i):
        return self.base[self.at[i]:self.at[i] + self.sizes[i]]

    def payloads(self):
        """the payloads, after checking that every byte outside them is still 0xA5"""
        host = self.base.cpu().numpy()
        outside = np.ones(host.size, dtype=bool)
        for start, n in zip(self.at, self.sizes):
            outside[start:start + n] = False
        assert (host[outside] == 0xA5).all(), "guard bytes were written"
        return [host[start:start + n] for start, n in zip(self.at, self.sizes)]


def layouts_of(regions, flip=0):
    """(pitch, pixel pointer offset) per region, two pairs in turn: a pointer that is a multiple of 16 with the pitch 8 w rounded
    up to 16 (`sc1 nt` stores in the fused kernel's full granules), and pointer + 8 with the pitch 8 w + 8 (plain stores)"""
    return [((BPP * w + 15) // 16 * 16, 0) if (i + flip) % 2 == 0 else (BPP * w + 8, 8) for i, (_, w, h) in enumerate(regions)]


def stream_of():
    import torch

    return torch.cuda.current_stream().cuda_stream


def run_regions(lib, dev, call, src_ptr, total, regions, layouts):
    """the images one region call writes: one arena for all of them"""
    import torch

    out = Arena(dev, [p * h for (_, _, h), (p, _) in zip(regions, layouts)], [off for _, off in layouts])
    arr = region_array(regions, out.ptrs, [p for p, _ in layouts])
    with torch.cuda.device(dev):
        assert call(src_ptr, total, arr, len(regions), stream_of()) == OK
    torch.cuda.synchronize()
    return out.payloads()


def run_single(lib, dev, src_ptr, total, regions, layouts, plain=False):
    """the images the single-image call writes for every region alone, all into one arena of the same layout"""
    import torch

    out = Arena(dev, [p * h for (_, _, h), (p, _) in zip(regions, layouts)], [off for _, off in layouts])
    with torch.cuda.device(dev):
        for (first, w, h), (pitch, _), ptr in zip(regions, layouts, out.ptrs):
            if plain:
                rc = lib.dxtlt_decode_bc6h_image_device(src_ptr + 16 * first, w, h, ptr, pitch, stream_of())
            else:
                rc = lib.dxtlt_untransform_decode_bc6h_image_device(src_ptr, total, first, w, h, ptr, pitch, stream_of())
            assert rc == OK
    torch.cuda.synchronize()
    return out.payloads()


def compare(got, alone, px, regions, layouts, tag=None):
    for i, (region, (pitch, off)) in enumerate(zip(regions, layouts)):
        assert np.array_equal(got[i], expected_buffer(px, region, pitch)), (tag, "numpy", i, region, pitch, off)
        assert np.array_equal(got[i], alone[i]), (tag, "single-image call", i, region, pitch, off)


def check_data(lib, dev, data, px, total, regions, layouts, *, plain=False, in_off=0, tag=None):
    """one region call on `data` at a pointer + in_off against the numpy statement and the single-image call, region by region"""
    src = Arena(dev, [data.size], [in_off], [data])
    call = lib.dxtlt_decode_bc6h_images_device if plain else lib.dxtlt_untransform_decode_bc6h_images_device
    got = run_regions(lib, dev, call, src.ptrs[0], total, regions, layouts)
    alone = run_single(lib, dev, src.ptrs[0], total, regions, layouts, plain)
    compare(got, alone, px, regions, layouts, tag)
    assert np.array_equal(src.payloads()[0], data.reshape(-1)), "the source changed"


def check_call(lib, dev, kind, total, regions, layouts, *, plain=False, in_off=0, seed=0, tag=None):
    x, px, t = reference(lib, kind, total, seed)
    check_data(lib, dev, x.reshape(-1) if plain else t, px, total, regions, layouts, plain=plain, in_off=in_off, tag=tag)


def shape_of(n):
    """an image of exactly n blocks whose last block column and row are clipped: as many block rows (at most 40) as divide n"""
    bh = max(d for d in range(1, 41) if n % d == 0)
    return 4 * (n // bh) - 1, 4 * bh - 2


# ---- the fused call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_256_chain_whose_small_levels_share_the_tail_part(lib, dev, kind):
    assert TOTAL_256 == 5463 and all(r[0] >= TOTAL_256 - TOTAL_256 % GRANULE for r in CHAIN_256[2:])
    for flip in (0, 1):
        check_call(lib, dev, kind, TOTAL_256, CHAIN_256, layouts_of(CHAIN_256, flip), tag=flip)


@pytest.mark.parametrize("faces", [2, 3])
@pytest.mark.parametrize("kind", list(KINDS))
def test_faces_of_a_128_chain(lib, dev, kind, faces):
    regions, total = (TWO_FACES, TOTAL_TWO) if faces == 2 else (THREE_FACES, TOTAL_THREE)
    assert [len(g) for _, g in groups_of(regions)] == ([PER_LAUNCH] if faces == 2 else [PER_LAUNCH, 8])
    for flip in (0, 1):
        check_call(lib, dev, kind, total, regions, layouts_of(regions, flip), tag=flip)


@pytest.mark.parametrize("base", [1024, 2048])
def test_a_boundary_at_every_phase_of_a_wave(lib, dev, base):
    """a 4p x 4 region of p blocks at `base` -- a main granule, the tail part -- then, behind a gap of 0, 1 or 2 blocks, 130 blocks
    of 65 block columns: the boundary and the gap pass every block of a wave's run.  In a full granule lane l stores blocks l / 2
    and 32 + l / 2 of the run, not the block it holds: a lookup keyed on the held block puts pixels in the wrong region here"""
    total = 2391
    assert total - total % GRANULE == 2048
    x, px, t = reference(lib, "interleaved", total)
    src = Arena(dev, [t.size], [0], [t])
    call = lib.dxtlt_untransform_decode_bc6h_images_device
    for p in range(1, 65):
        for gap in (0, 1, 2):
            regions = [(base, 4 * p, 4), (base + p + gap, 260, 8)]
            assert region_end(regions[1]) <= total and blocks_of(260, 8) == 130
            layouts = layouts_of(regions, p + gap)
            got = run_regions(lib, dev, call, src.ptrs[0], total, regions, layouts)
            alone = run_single(lib, dev, src.ptrs[0], total, regions, layouts)
            compare(got, alone, px, regions, layouts, (p, gap))
    assert np.array_equal(src.payloads()[0], t), "the transformed buffer changed"


def test_store_and_clip_classes_per_region_in_one_call(lib, dev):
    """pixel pointers +0 and +8, pitches 8w, 8w + 8 and 8w + 16, whole and clipped blocks, all in one call: the streaming-or-plain
    choice and the clipping are the region's, also where regions of both kinds meet inside one wave"""
    sizes = [(1, 1), (7, 5), (64, 64), (260, 36)]
    combos = [(0, 0), (8, 0), (0, 16), (8, 8), (0, 8), (8, 16)]   # (pixel pointer offset, pitch - 8w)
    regions, layouts, at = [], [], 7
    for off, extra in combos:
        for w, h in sizes:
            regions.append((at, w, h))
            layouts.append((BPP * w + extra, off))
            at += blocks_of(w, h)
    total = 5463
    assert at <= total and len(regions) == 24
    # some wave holds whole blocks of a region with streaming stores and whole blocks of one with plain stores
    kind = np.full(total, -1)   # 1: a whole block of a streaming-store region, 0: of a plain-store region, -1: clipped or in no region
    for (first, w, h), (pitch, off) in zip(regions, layouts):
        bw, bh = (w + 3) // 4, (h + 3) // 4
        whole = np.zeros((bh, bw), dtype=bool)
        whole[:h // 4, :w // 4] = True
        kind[first:first + bw * bh] = np.where(whole.reshape(-1), int(off % 16 == 0 and pitch % 16 == 0), -1)
    waves = kind[:total - total % GRANULE].reshape(-1, 64)          # full granules: where the choice between the two exists
    assert ((waves == 1).any(axis=1) & (waves == 0).any(axis=1)).any()
    check_call(lib, dev, "interleaved", total, regions, layouts)


@pytest.mark.parametrize("total", TOTALS)
def test_every_total_whole_with_gaps_and_with_empty_regions(lib, dev, total):
    lists = [[(0,) + shape_of(total)]]
    if total >= 5:
        inner = total - 2                    # blocks 0 and total - 1 stay in gaps, and so does one in the middle
        n1 = inner // 2
        n2 = inner - n1 - 1
        lists.append([(1,) + shape_of(n1), (2 + n1,) + shape_of(n2)])
        lists.append([(2**63, 0, 7), (1,) + shape_of(n1), (2**63, 5, 0), (0, 0, 0), (2 + n1,) + shape_of(n2), (3, 9, 0)])
    else:
        lists.append([(5, 0, 3), (0,) + shape_of(total), (2**63, 0, 0)])
    for k, regions in enumerate(lists):
        assert all(blocks_of(w, h) == 0 or region_end((f, w, h)) <= total for f, w, h in regions)
        for flip in (0, 1):
            check_call(lib, dev, "interleaved", total, regions, layouts_of(regions, flip), tag=(k, flip))


@pytest.mark.parametrize("cls", range(ref.CLASSES))
def test_the_chain_on_a_buffer_of_one_class(lib, dev, cls):
    x, px, t = reference_of(lib, ("class", cls), lambda: ref.single_class_blocks(TOTAL_256, cls, 60 + cls))
    check_data(lib, dev, t, px, TOTAL_256, CHAIN_256, layouts_of(CHAIN_256, cls), tag=cls)


def test_transformed_buffer_at_an_address_that_is_no_multiple_of_16(lib, dev):
    """dxtlt_transform_bc6h_range_device accepts any address: the transformed buffer is made on the device at one that is no
    multiple of 16, and its chain decoded from there"""
    import torch

    total, regions = TOTAL_256, CHAIN_256
    x, px, t = reference(lib, "balanced", total)
    layouts = layouts_of(regions)
    for in_off in (1, 8):
        src = Arena(dev, [x.size], [0], [x])
        mid = Arena(dev, [x.size], [in_off])
        with torch.cuda.device(dev):
            assert lib.dxtlt_transform_bc6h_range_device(False, src.ptrs[0], mid.ptrs[0], total, 0, total, stream_of()) == OK
        got = run_regions(lib, dev, lib.dxtlt_untransform_decode_bc6h_images_device, mid.ptrs[0], total, regions, layouts)
        alone = run_single(lib, dev, mid.ptrs[0], total, regions, layouts)
        assert np.array_equal(mid.payloads()[0], t), in_off
        compare(got, alone, px, regions, layouts, in_off)


# ---- the other calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", [0, 8])
@pytest.mark.parametrize("case", ["chain", "two faces"])
def test_block_array_call(lib, dev, case, in_off):
    regions, total = (CHAIN_256, TOTAL_256) if case == "chain" else (TWO_FACES, TOTAL_TWO)
    for flip in (0, 1):
        check_call(lib, dev, "interleaved", total, regions, layouts_of(regions, flip), plain=True, in_off=in_off, tag=flip)


def test_host_call(lib):
    # the chain; level 1 in a gap and an empty region in the list; three regions 9 pixels wide, the middle one empty, the first from
    # the main part into the tail part: rows of 72 bytes, staged 80 apart
    for total, regions in ((TOTAL_256, CHAIN_256), (TOTAL_256, [CHAIN_256[0], (2**63, 0, 7)] + CHAIN_256[2:]),
                           (1100, [(1000, 9, 50), (2**63, 0, 7), (1050, 9, 14)])):
        x, px, t = reference(lib, "interleaved", total)
        pitches = [BPP * w + 24 for _, w, h in regions]
        hosts = [np.full(GUARD + p * h + GUARD, 0xA5, dtype=np.uint8) for (_, w, h), p in zip(regions, pitches)]
        arr = region_array(regions, [b.ctypes.data + GUARD for b in hosts], pitches)
        assert all((b.ctypes.data + GUARD) % 8 == 0 for b in hosts)
        assert lib.dxtlt_untransform_decode_bc6h_images(t.ctypes.data, t.size, arr, len(regions)) == OK
        for i, (region, p, host) in enumerate(zip(regions, pitches, hosts)):
            n = p * region[2]
            assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n:] == 0xA5).all(), (total, i)
            assert np.array_equal(host[GUARD:GUARD + n], expected_buffer(px, region, p)), (total, i)


def test_python_wrappers_on_tensors_and_host_buffers(pkg, lib, dev):
    import torch

    from dxt_lossless_transform_amd import image

    x, px, t = reference(lib, "interleaved", TOTAL_256)
    regions, total = image.mip_chain(256, 256, 9)
    assert (regions, total) == (CHAIN_256, TOTAL_256)
    want = [expected_buffer(px, r, BPP * r[1]) for r in regions]
    outs = image.untransform_decode_bc6h_images(torch.from_numpy(t.copy()).to(dev), regions)
    torch.cuda.synchronize()
    assert all(o.is_cuda and o.dtype == torch.uint8 and np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, want))
    # the documented view: (height, width, 4) half floats
    for o, (first, w, h) in zip(outs, regions):
        halves = o.view(torch.float16).reshape(h, w, 4).cpu().numpy().view(np.uint16)
        assert np.array_equal(halves, ref.image_of(px[first:first + blocks_of(w, h)], w, h))
    outs = image.untransform_decode_bc6h_images(t, regions)
    assert all(isinstance(o, np.ndarray) and np.array_equal(o, w) for o, w in zip(outs, want))
    outs = image.decode_bc6h_images(torch.from_numpy(x.reshape(-1).copy()).to(dev), regions)
    torch.cuda.synchronize()
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, want))
    # outputs and pitches of the caller's
    pitches = [BPP * r[1] + 16 for r in regions[3:]]
    mine = [torch.full((p * r[2],), 0xA5, dtype=torch.uint8, device=dev) for r, p in zip(regions[3:], pitches)]
    back = image.untransform_decode_bc6h_images(torch.from_numpy(t.copy()).to(dev), regions[3:], outs=mine, pitches=pitches)
    torch.cuda.synchronize()
    assert all(b is m for b, m in zip(back, mine))
    assert all(np.array_equal(m.cpu().numpy(), expected_buffer(px, r, p)) for m, r, p in zip(mine, regions[3:], pitches))
    # ... and on host buffers
    hosts = [np.full(p * r[2], 0xA5, dtype=np.uint8) for r, p in zip(regions[3:], pitches)]
    back = image.untransform_decode_bc6h_images(t, regions[3:], outs=hosts, pitches=pitches)
    assert all(b is m for b, m in zip(back, hosts))
    assert all(np.array_equal(m, expected_buffer(px, r, p)) for m, r, p in zip(hosts, regions[3:], pitches))


def test_fused_call_replays_from_a_hip_graph_with_the_table_frozen_at_capture(lib, dev):
    import torch

    regions, total = TWO_FACES, TOTAL_TWO      # one group over both main granules and the tail part: two launches
    layouts = layouts_of(regions)
    x, px, t = reference(lib, "interleaved", total)
    src = Arena(dev, [t.size], [0], [t])
    out = Arena(dev, [p * h for (_, _, h), (p, _) in zip(regions, layouts)], [off for _, off in layouts])
    arr = region_array(regions, out.ptrs, [p for p, _ in layouts])

    def work():
        rc = lib.dxtlt_untransform_decode_bc6h_images_device(src.ptrs[0], total, arr, len(regions), torch.cuda.current_stream(dev).cuda_stream)
        assert rc == OK

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        work()                                    # warm-up outside capture (module load, first launch)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    # the table is the graph's by now: the caller's array is overwritten.  New blocks in the same buffer, the outputs poisoned
    # again: only a replay with the captured table can produce the right images
    for r in arr:
        r.first_block, r.width, r.height, r.pixels, r.pitch = 0, 0, 0, None, 0
    x2, px2, t2 = reference(lib, "balanced", total, seed=1)
    assert not np.array_equal(x, x2)
    src.view(0).copy_(torch.from_numpy(t2.copy()).to(dev))
    out.base.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize(dev)
    got = out.payloads()
    for i, (region, (pitch, _)) in enumerate(zip(regions, layouts)):
        assert np.array_equal(got[i], expected_buffer(px2, region, pitch)), i
    assert np.array_equal(src.payloads()[0], t2)
