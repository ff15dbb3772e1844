"""The images of many BC6H transformed buffers in one call on the MI355X (include/dxtlt_bc6h_image.h,
dxtlt_untransform_decode_bc6h_images_batch_device).  Every image is compared byte for byte with the numpy statement of
tests/bc6h_decode_ref.py AND with the bytes dxtlt_untransform_decode_bc6h_images_device writes for the item alone.  All images of a
call live in one arena prefilled with 0xA5 -- the guard bytes around and between them, the pitch padding and the pixels a clipped
block does not have must still be 0xA5 afterwards -- and the single calls write into a second arena of the same layout: the two
arenas are equal byte for byte.  The sources live in a guarded arena too and are unchanged.  Transformed buffers come from
dxtlt_transform_bc6h on the three kinds of data of tests/test_bc6h_image_regions_gpu.py (the reserved classes ride along as they
do there); the largest is 5463 blocks."""
import numpy as np
import pytest

import bc6h_decode_ref as ref
from bc6h_image_batch_common import Item, batch_items, item_layouts, load, plan, plan_of
from bc6h_image_regions_common import BPP, CHAIN_256, GRANULE, OK, PER_LAUNCH, TOTAL_256, blocks_of, groups_of, region_end
from image_regions_common import mip_chain

pytestmark = pytest.mark.gpu

GUARD = 256
TOTALS = (1, 37, 1023, 1024, 1025, 2391, 5463)
KINDS = {"balanced": ref.mode_balanced_blocks, "wave_uniform": ref.wave_uniform_blocks, "interleaved": ref.interleaved_class_blocks}
CHAIN_64, TOTAL_64 = mip_chain(64, 64, 7)
assert TOTAL_64 == 343


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


_cache = {}


def reference(lib, kind, total, seed=0):
    """(their pixels (total, 16, 4) uint16, the transformed buffer) of a whole array of blocks, computed once and shared"""
    key = (kind, total, seed)
    if key not in _cache:
        x = KINDS[kind](total, 500 + seed)
        t = np.zeros(x.size, dtype=np.uint8)
        assert lib.dxtlt_transform_bc6h(x.ctypes.data, t.ctypes.data, x.size) == OK
        px = ref.decode_blocks(x)
        for a in (t, px):
            a.setflags(write=False)
        _cache[key] = (px, t)
    return _cache[key]


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

    def __init__(self, dev, sizes, offs, data=None):
        import torch

        self.at, end = [], 0
        for n, off in zip(sizes, offs):
            start = (end + GUARD + 255) // 256 * 256 + off
            self.at.append(start)
            end = start + n
        self.sizes = list(sizes)
        host = np.full(end + GUARD, 0xA5, dtype=np.uint8)
        if data is not None:
            for start, d in zip(self.at, data):
                host[start:start + d.size] = d
        self.base = torch.from_numpy(host).to(dev)
        assert self.base.data_ptr() % 256 == 0
        self.ptrs = [self.base.data_ptr() + start for start in self.at]

    def host(self):
        return self.base.cpu().numpy()

    def payloads(self, host=None):
        """the payloads, after checking that every byte outside them is still 0xA5"""
        host = self.host() if host is None else host
        outside = np.ones(host.size, dtype=bool)
        for start, n in zip(self.at, self.sizes):
            outside[start:start + n] = False
        assert (host[outside] == 0xA5).all(), "guard bytes were written"
        return [host[start:start + n] for start, n in zip(self.at, self.sizes)]


def aligned_pitch(width):
    return (BPP * width + 15) // 16 * 16 + 16


def layouts_of(regions, flip=0):
    """(pitch, pixel pointer offset) per region, two forms in turn: a pointer that is a multiple of 16 with the pitch 8 w rounded up
    to 16 plus 16 (streaming stores in a full granule), and pointer + 8 with the pitch 8 w + 8 (plain stores)"""
    return [(aligned_pitch(w), 0) if (i + flip) % 2 == 0 else (BPP * w + 8, 8) for i, (_, w, h) in enumerate(regions)]


def shape_of(n):
    """an image of exactly n blocks whose last block column and row are clipped: as many block rows (at most 40) as divide n"""
    bh = max(d for d in range(1, 41) if n % d == 0)
    return 4 * (n // bh) - 1, 4 * bh - 2


class Batch:
    """The sources and the outputs of `items` on the device: one source per distinct item (items with the same `share` key read
    one buffer), two output arenas of one layout -- `out` for the batch call, `alone` for the single calls"""

    def __init__(self, lib, dev, items):
        self.lib, self.dev, self.items = lib, dev, items
        self.refs = [reference(lib, it.kind, it.total, it.seed) if it.total else (None, np.zeros(0, np.uint8)) for it in items]
        owner, self.source_of = {}, []
        for i, it in enumerate(items):
            key = ("own", i) if it.share is None else it.share
            self.source_of.append(owner.setdefault(key, len(owner)))
        first_of = {s: self.source_of.index(s) for s in set(self.source_of)}
        order = sorted(first_of)
        self.src = Arena(dev, [self.refs[first_of[s]][1].size for s in order], [items[first_of[s]].in_off for s in order],
                         [self.refs[first_of[s]][1] for s in order])
        self.src_data = [self.refs[first_of[s]][1] for s in order]
        sizes, offs = [], []
        for it in items:
            for (_, w, h), (pitch, off) in zip(it.regions, item_layouts(it)):
                sizes.append(pitch * h)
                offs.append(off)
        self.out, self.alone = Arena(dev, sizes, offs), Arena(dev, sizes, offs)
        self.keep = []

    def pointers(self, arena):
        ptrs, at = [], 0
        for it in self.items:
            ptrs.append(arena.ptrs[at:at + len(it.regions)])
            at += len(it.regions)
        return ptrs

    def array(self, arena):
        return batch_items(self.items, [self.src.ptrs[s] for s in self.source_of], self.pointers(arena), self.keep)

    def call(self, stream=None):
        """enqueues the batch call"""
        import torch

        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        assert self.lib.dxtlt_untransform_decode_bc6h_images_batch_device(self.array(self.out), len(self.items), stream) == OK, \
            self.lib.dxtlt_last_error()

    def check(self):
        """after a synchronise: the batch call's arena against the numpy statement, the guards, the single calls and the sources"""
        import torch

        got_host = self.out.host()
        got = self.out.payloads(got_host)
        at = 0
        for i, it in enumerate(self.items):
            for k, (region, (pitch, off)) in enumerate(zip(it.regions, item_layouts(it))):
                assert np.array_equal(got[at], expected_buffer(self.refs[i][0], region, pitch)), ("numpy", i, k, region, pitch, off)
                at += 1
        arr = self.array(self.alone)
        for i, it in enumerate(self.items):
            rc = self.lib.dxtlt_untransform_decode_bc6h_images_device(arr[i].d_transformed, it.total, arr[i].regions, len(it.regions),
                                                                      torch.cuda.current_stream().cuda_stream)
            assert rc == OK, (i, self.lib.dxtlt_last_error())
        torch.cuda.synchronize()
        assert np.array_equal(got_host, self.alone.host()), "the batch call and the single calls wrote different bytes"
        for mine, data in zip(self.src.payloads(), self.src_data):
            assert np.array_equal(mine, data), "a source changed"


def check_batch(lib, dev, items):
    import torch

    b = Batch(lib, dev, items)
    b.call()
    torch.cuda.synchronize()
    b.check()
    return b


def whole(total, kind="interleaved", seed=0, flip=0, **kw):
    """an item whose one region is the whole buffer, of clipped shape"""
    regions = [(0,) + shape_of(total)]
    return Item(total, regions, kind, seed, layouts=layouts_of(regions, flip), **kw)


def chain_256(kind="interleaved", seed=0, flip=0, **kw):
    return Item(TOTAL_256, list(CHAIN_256), kind, seed, layouts=layouts_of(CHAIN_256, flip), **kw)


def chain_64(kind="interleaved", seed=0, flip=0, **kw):
    return Item(TOTAL_64, list(CHAIN_64), kind, seed, layouts=layouts_of(CHAIN_64, flip), **kw)


# ---- the mixed batch --------------------------------------------------------------------------------------------------------
def test_every_total_and_the_256_chain_of_every_data_kind_in_one_call(lib, dev):
    items = []
    for k, kind in enumerate(KINDS):
        for j, total in enumerate(TOTALS):
            items.append(whole(total, kind, flip=j + k))
        items.append(chain_256(kind, flip=k))
    got = plan(lib, items)
    assert got == plan_of(items) and got[0][7] == 3 * (1 + 1 + 2 + 5 + 5) and got[0][8] == 3 * 7
    check_batch(lib, dev, items)


# ---- the lookup -------------------------------------------------------------------------------------------------------------
def test_150_items_of_one_granule_and_a_tail_each(lib, dev):
    """64 consecutive workgroups span 64 entries: the longest scan behind a coarse index entry.  (Four buffers of data serve all
    items: what differs from item to item is the entry.)"""
    sizes = (1025, 1366, 1707, 2047)
    items = [whole(sizes[i % 4], list(KINDS)[i % 3], flip=i, share=(sizes[i % 4], i % 3)) for i in range(150)]
    got = plan(lib, items)
    assert got == plan_of(items) and all(e[4] == 1 and e[5] == i and e[6] == i for i, e in enumerate(got)) and got[0][7:] == (150, 150)
    assert 150 % 64 != 0
    check_batch(lib, dev, items)


def test_40_chains_whose_coarse_index_entries_land_mid_entry(lib, dev):
    items = [chain_256(list(KINDS)[i % 3], seed=i % 2, flip=i) for i in range(40)]
    got = plan(lib, items)
    assert got[0][7:] == (200, 40) and 200 % 64 != 0 and [e[5] for e in got] == list(range(0, 200, 5))
    assert all(any(e[5] < 64 * k < e[5] + e[4] for e in got) for k in (1, 2, 3))      # workgroups 64, 128, 192: inside an entry
    check_batch(lib, dev, items)


def test_300_tail_only_chains_launch_no_granule_kernel(lib, dev):
    items = [chain_64(list(KINDS)[i % 3], seed=i % 2, flip=i) for i in range(300)]
    got = plan(lib, items)
    assert len(got) == 300 and all(e[4] == 0 and e[6] == i for i, e in enumerate(got)) and got[0][7:] == (0, 300)
    check_batch(lib, dev, items)


def test_a_main_only_item_between_two_ordinary_ones(lib, dev):
    main_only = Item(TOTAL_256, CHAIN_256[:2], "balanced", layouts=layouts_of(CHAIN_256[:2], 1))
    inside = Item(2391, [(1500, 64, 16)], "wave_uniform")
    items = [chain_256(), main_only, chain_64(), inside, whole(2391)]
    got = plan(lib, items)
    assert [e[6] for e in got] == [0, -1, 1, -1, 2] and [e[4] for e in got] == [5, 5, 0, 1, 2]
    check_batch(lib, dev, items)


def test_an_item_of_two_entries_whose_groups_share_a_granule(lib, dev):
    regions = [(205 * k, 164, 20) for k in range(20)]
    assert [len(g) for _, g in groups_of(regions)] == [PER_LAUNCH, 4] and 205 * 16 // GRANULE == 3
    two = Item(4101, regions, "balanced", layouts=layouts_of(regions))
    items = [chain_64(), two, chain_256(flip=1)]
    got = plan(lib, items)
    assert [(e[0], e[3], e[4]) for e in got] == [(0, 0, 0), (1, 0, 4), (1, 3, 1), (2, 0, 5)]
    check_batch(lib, dev, items)


@pytest.mark.parametrize("base", [1024, 2048])
def test_a_boundary_at_every_phase_of_a_wave(lib, dev, base):
    """a 4p x 4 region of p blocks at `base` -- a main granule, the tail part -- then, behind a gap of 0, 1 or 2 blocks, 130 blocks
    of 65 block columns: the boundary and the gap pass every block of a wave's run; all 192 items in one call over one source, an
    ordinary item on either side of each.  In a full granule lane l stores blocks l / 2 and 32 + l / 2 of the run, not the block it
    holds: a lookup keyed on the held block puts pixels in the wrong region here, and an entry applied to the neighbour's workgroup
    puts the ordinary item's pixels where the boundary item's belong"""
    total = 2391
    assert total - total % GRANULE == 2048
    items = [chain_64(share="ordinary")]
    for p in range(1, 65):
        for gap in (0, 1, 2):
            regions = [(base, 4 * p, 4), (base + p + gap, 260, 8)]
            assert region_end(regions[1]) <= total and blocks_of(260, 8) == 130
            items.append(Item(total, regions, "interleaved", layouts=layouts_of(regions, p + gap), share="boundary"))
            items.append(chain_64(share="ordinary", flip=p))
    assert len(items) == 1 + 2 * 192
    check_batch(lib, dev, items)


def test_gaps_empty_regions_and_an_all_empty_item(lib, dev):
    items = []
    for total in (37, 1025, 5463):
        inner = total - 2                    # blocks 0 and total - 1 stay in gaps, and so does one in the middle
        n1 = inner // 2
        n2 = inner - n1 - 1
        regions = [(2**63, 0, 7), (1,) + shape_of(n1), (2**63, 5, 0), (0, 0, 0), (2 + n1,) + shape_of(n2), (3, 9, 0)]
        items.append(Item(total, regions, "interleaved", layouts=layouts_of(regions, total)))
        items.append(Item(total, [(5, 0, 3), (2**63, 0, 0)], "interleaved", seed=1))
    items.append(Item(0, []))
    items.append(Item(TOTAL_256, [CHAIN_256[0], (2**63, 0, 7), CHAIN_256[2], (5400, 0, 0), CHAIN_256[5]], "balanced"))
    assert sorted({e[0] for e in plan(lib, items)}) == [0, 2, 4, 7]
    check_batch(lib, dev, items)


def test_two_items_on_one_buffer_with_disjoint_images(lib, dev):
    even = Item(TOTAL_256, CHAIN_256[0::2], "balanced", layouts=layouts_of(CHAIN_256[0::2]), share="chain")
    odd = Item(TOTAL_256, CHAIN_256[1::2], "balanced", layouts=layouts_of(CHAIN_256[1::2], 1), share="chain")
    b = check_batch(lib, dev, [even, chain_64(), odd])
    assert len(b.src.sizes) == 2


def test_store_and_clip_classes_per_region_in_one_call(lib, dev):
    """pixel pointers +0 and +8, pitches 8w, 8w + 8 and 8w + 16, whole and clipped blocks, in one item and across items: the
    streaming-or-plain choice and the clipping are the region's, also where regions of both kinds meet inside one wave"""
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
        full = np.zeros((bh, bw), dtype=bool)
        full[:h // 4, :w // 4] = True
        kind[first:first + bw * bh] = np.where(full.reshape(-1), int(off % 16 == 0 and pitch % 16 == 0), -1)
    waves = kind[:total - total % GRANULE].reshape(-1, 64)          # full granules: where the choice between the two exists
    assert ((waves == 1).any(axis=1) & (waves == 0).any(axis=1)).any()
    items = [Item(total, regions, "interleaved", layouts=layouts)]
    for k, (off, extra) in enumerate(combos):
        for n in (1025, 37):
            w, h = shape_of(n) if k % 2 else (4 * n, 4)
            items.append(Item(n, [(0, w, h)], "balanced", layouts=[(BPP * w + extra, off)]))
    check_batch(lib, dev, items)


@pytest.mark.parametrize("in_off", [16, 1, 4, 8, 20])
def test_transformed_buffers_at_any_address(lib, dev, in_off):
    items = [chain_256(in_off=in_off), chain_64("balanced", in_off=in_off), whole(1025, "wave_uniform", in_off=in_off),
             chain_256("balanced", flip=1)]
    check_batch(lib, dev, items)


# ---- streams, the ring, Python ----------------------------------------------------------------------------------------------
def test_a_side_stream(lib, dev):
    import torch

    b = Batch(lib, dev, [chain_256("balanced"), chain_64(), whole(2391, "wave_uniform")])
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        b.call(side.cuda_stream)
    side.synchronize()
    b.check()


def test_five_calls_back_to_back_reuse_the_ring(lib, dev):
    """more calls than the table ring has slots, one synchronise behind them all"""
    import torch

    batches = [Batch(lib, dev, [chain_256(list(KINDS)[k % 3], seed=k % 2, flip=k), chain_64(seed=k % 2), whole(TOTALS[k + 2], flip=k)])
               for k in range(5)]
    for b in batches:
        b.call()
    torch.cuda.synchronize()
    for b in batches:
        b.check()


def test_python_wrapper_on_tensors(pkg, lib, dev):
    import torch

    from dxt_lossless_transform_amd import image

    px, t = reference(lib, "interleaved", TOTAL_256)
    px2, t2 = reference(lib, "balanced", TOTAL_64)
    regions, total = image.mip_chain(256, 256, 9)
    assert (regions, total) == (CHAIN_256, TOTAL_256)
    pitches = [BPP * r[1] + 16 for r in CHAIN_64[2:]]
    mine = [torch.full((p * r[2],), 0xA5, dtype=torch.uint8, device=dev) for r, p in zip(CHAIN_64[2:], pitches)]
    padded = torch.cat([torch.from_numpy(t2.copy()), torch.zeros(32, dtype=torch.uint8)]).to(dev)
    outs = image.untransform_decode_bc6h_images_batch([
        (torch.from_numpy(t.copy()).to(dev), regions),
        (padded, CHAIN_64[2:], {"total_blocks": TOTAL_64, "outs": mine, "pitches": pitches}),
        (torch.from_numpy(t2.copy()).to(dev), [], None)])
    torch.cuda.synchronize()
    assert [len(o) for o in outs] == [9, 5, 0]
    # the default pitch is 8 * width, the outputs uint8
    assert all(o.is_cuda and o.dtype == torch.uint8 and np.array_equal(o.cpu().numpy(), expected_buffer(px, r, BPP * r[1]))
               for o, r in zip(outs[0], regions))
    assert all(b is m for b, m in zip(outs[1], mine))
    assert all(np.array_equal(m.cpu().numpy(), expected_buffer(px2, r, p)) for m, r, p in zip(mine, CHAIN_64[2:], pitches))
    with pytest.raises(TypeError):
        image.untransform_decode_bc6h_images_batch([(torch.from_numpy(t.copy()).to(dev), regions, {"mode": 1})])
    with pytest.raises(pkg.DeviceError) as err:
        image.untransform_decode_bc6h_images_batch([(torch.from_numpy(t.copy()).to(dev), regions), (padded, [(340, 8, 8)], {"total_blocks": TOTAL_64})])
    assert "item 1:" in str(err.value)
