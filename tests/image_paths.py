"""The path census of the image decode sinks (docs/IMAGE_DECODE.md, "What the tests reach"): for a case -- one call of an image
decoder, as plain data -- which store and lookup path every block of every region takes.  Plain Python, no device.  It is a second,
independent statement of the rules of csrc/image_kernels.hip (PixelSink, ChannelSink, the plain decoders), csrc/image_region_sinks.h
(RegionPixelSinkOf, RegionChannelSinkOf), csrc/image_regions_kernels.hip (the plain region decoders) and csrc/image_store.h; it
calls none of them.  Only the launch shape is asked of the library, through the planning hooks that have tests of their own
(dxtlt_debug_plan_transform, dxtlt_debug_plan_image_batch).  tests/test_image_paths_layout.py proves what the case lists reach,
tests/test_image_paths_gpu.py runs them and names the cell of a wrong byte.

A cell is (tile kind, wave path, lane path, store class, clip class):

  tile kind    "aligned" / "shifted": a full tile of launch kind 0 / 2 (the sink's `store`: all lanes, BC1 with the eight-bpermute
               exchange); "edge": the one ragged tile of a launch (`store_edge`: a lane keeps its own blocks);
               "plain vector" / "plain bytes": the plain decoders, block pointer on / off a multiple of the block size.
  wave path    "single": the single-image kernels have no lookup; "uniform": region_of_run found the wave's whole run in one region;
               "per lane": it did not, every lane looks with region_of_block; "edge": the edge tile never asks for the run.
  lane path    BC1 - BC3: "exchange" (BC1, full tile: lane l holds blocks l and 64 + l of the wave) or "own".
               BC4 / BC5: "rows8" (the lane's 8 bytes per pixel row in one store: store_channel_lane's condition) or "alone" (every
               block for itself).  BC4 also has `pair`, what became of the lane's two blocks: "same region", "two regions",
               "first only" (the second is in a gap, or the vector holds one block), "second only", "neither".
  store class  the alignment class of the block's image, (pixel pointer | pitch): BC1 - BC3 "stream16" (multiple of 16: streaming
               16-byte stores) / "plain16" (4-byte aligned 16-byte stores); BC4 / BC5 "stream8" (16) / "plain8" (8), which are the
               rows8 stores and for a block alone mean dwords, "dwords" (4), "halfwords" (2), "bytes" (odd, BC4 only).
  clip class   "whole", or clipped by the image's "right" edge, "bottom" edge, or both ("corner"): written pixel by pixel.

Lane-to-block assignment.  A wave is 64 lanes and holds W = 128 (BC1, BC4) or 64 consecutive blocks; tile k of a launch covers
blocks [k T, (k + 1) T) of the launch's range, T = threads * 16 / block bytes, its wave j the blocks [j W, (j + 1) W) of the tile.
Lane t of a tile holds blocks PV t .. PV t + PV - 1 (PV = 2 for BC1 and BC4).  The plain decoders: lane i of the launch holds block
i (BC1 - BC3, BC1 too: a wave is 64 blocks there) or blocks PV i .. (BC4 / BC5) of the range, counted from the first region's first
block; lanes past the range leave, and the run a wave asks about is still the blocks of all its 64 lanes."""
from __future__ import annotations

import collections

from image_batch_common import TILE, Item, plan as plan_batch
from image_regions_common import BLOCK, BPP, FMT_ID, PER_LAUNCH, PlannedLaunch, blocks_of

ENTRIES = ("single", "plain single", "regions", "plain regions", "batch")
RGBA = ("bc1", "bc2", "bc3")
PV = {"bc1": 2, "bc2": 1, "bc3": 1, "bc4": 2, "bc5": 1}     # blocks in a lane's 16-byte vector
WAVE = {fmt: 64 * PV[fmt] for fmt in PV}                      # blocks of a wave
PLAN_ADDRESS = 0x7F00_0000_0000                               # stands for an allocation on a 256-byte address

# entry: one of ENTRIES.  in_off: the source pointer modulo 256.  regions: [(first_block, width, height)], exactly one for the
# single-image entries.  out_offs / pitches: per region, the pixel pointer modulo 256 and the pitch.  seed: of the blocks.
Case = collections.namedtuple("Case", "entry fmt settings in_off total regions out_offs pitches seed name")
# pair, slot: BC4 only -- what became of the lane's two blocks, and which of the two (0, 1) this block is
Cell = collections.namedtuple("Cell", "tile wave lane store clip pair slot")


def cell5(cell):
    return tuple(cell[:5])


def store_class(fmt, address, pitch):
    al = address | pitch
    if fmt in RGBA:
        return "stream16" if al % 16 == 0 else "plain16"
    for multiple, name in ((16, "stream8"), (8, "plain8"), (4, "dwords"), (2, "halfwords")):
        if al % multiple == 0:
            return name
    return "bytes"


def place(width, height, local):
    """(block column, pixel columns, pixel rows inside the image) of block `local` of a width x height image"""
    by, bx = divmod(local, (width + 3) // 4)
    return bx, min(4, width - 4 * bx), min(4, height - 4 * by)


def clip_class(cols, rows):
    return {(True, True): "whole", (False, True): "right", (True, False): "bottom", (False, False): "corner"}[(cols == 4, rows == 4)]


def as_item(case):
    return Item(case.fmt, case.settings, case.total, list(case.regions), case.in_off, case.seed, list(case.pitches), list(case.out_offs))


class Census:
    """cells[k][b]: the Cell of block b of region k; dropped: (tile kind, wave path, "dropped" / "neither") of lanes whose blocks lie
    in no region; kinds: the launch kinds of the plan, per group of regions"""

    def __init__(self, case):
        self.case = case
        self.cells = [[None] * blocks_of(w, h) for _, w, h in case.regions]
        self.dropped = set()
        self.kinds = []

    def mark(self, region, local, cell):
        assert self.cells[region][local] is None, (self.case.name, region, local, "a block is written twice")
        self.cells[region][local] = cell

    def all_cells(self):
        return [c for cells in self.cells for c in cells]


# ---- the lookups of image_regions.h over a group: [(index in the case's list, first block, blocks)] ----------------------------
def region_of_run(group, b, n):
    for k, first, blocks in group:
        if 0 <= b - first < blocks and n <= blocks - (b - first):
            return k, first
    return None


def region_of_block(group, b):
    for k, first, blocks in group:
        if 0 <= b - first < blocks:
            return k, first
    return None


def groups_of(regions, first_region=0, count=None):
    """the non-empty regions from `first_region` on in groups of at most sixteen (`count`: only that many regions, one group)"""
    groups, group = [], []
    for k in range(first_region, len(regions)):
        first, w, h = regions[k]
        if w == 0 or h == 0:
            continue
        group.append((k, first, blocks_of(w, h)))
        if len(group) == (count or PER_LAUNCH):
            groups.append(group)
            group = []
            if count:
                return groups
    if group:
        groups.append(group)
    return groups


# ---- the stores of image_store.h ------------------------------------------------------------------------------------------------
def put_pixels(cen, group, tile, wave, lane, run, b):
    """RegionPixelSinkOf::put / decode_and_store: one BC1 - BC3 block `b` of the buffer"""
    case = cen.case
    found = run if run is not None else region_of_block(group, b)
    if found is None:
        cen.dropped.add((tile, wave, "dropped"))
        return
    k, first = found
    _, width, height = case.regions[k]
    _, cols, rows = place(width, height, b - first)
    cen.mark(k, b - first, Cell(tile, wave, lane, store_class(case.fmt, case.out_offs[k], case.pitches[k]), clip_class(cols, rows), None, None))


def channel_lane(cen, tile, wave, k, local, have, pair, slot=0):
    """store_channel_lane: the first `have` blocks of a lane's vector, the first of them block `local` of region k"""
    case = cen.case
    pv = PV[case.fmt]
    _, width, height = case.regions[k]
    al = case.out_offs[k] | case.pitches[k]
    bx, _, rows = place(width, height, local)
    rows8 = have == pv and al % 8 == 0 and bx % pv == 0 and 4 * (bx + pv) <= width and rows == 4
    for j in range(have):
        _, c, r = place(width, height, local + j)
        assert not rows8 or (c, r) == (4, 4)
        cen.mark(k, local + j, Cell(tile, wave, "rows8" if rows8 else "alone", store_class(case.fmt, case.out_offs[k], case.pitches[k]),
                                    clip_class(c, r), pair, None if pair is None else slot + j))


def put_channels(cen, group, tile, wave, run, b, have):
    """ChannelSink / RegionChannelSinkOf::put: the first `have` blocks of a lane's vector, the first of them block `b` of the buffer"""
    fmt = cen.case.fmt
    if run is not None:                       # one image for the whole wave: the single-image kernels' store
        k, first = run
        channel_lane(cen, tile, wave, k, b - first, have, None if fmt == "bc5" else "same region" if have == 2 else "first only")
        return
    r0 = region_of_block(group, b)
    if fmt == "bc5":
        if r0 is None:
            cen.dropped.add((tile, wave, "dropped"))
        else:
            channel_lane(cen, tile, wave, r0[0], b - r0[1], 1, None)
        return
    r1 = region_of_block(group, b + 1) if have == 2 else None
    together = r0 is not None and r1 == r0
    pair = ("same region" if together else "two regions" if r0 is not None and r1 is not None else "first only" if r0 is not None
            else "second only" if r1 is not None else "neither")
    if r0 is not None:
        channel_lane(cen, tile, wave, r0[0], b - r0[1], 2 if together else 1, pair)
    if r1 is not None and not together:
        channel_lane(cen, tile, wave, r1[0], b + 1 - r1[1], 1, pair, 1)
    if pair == "neither":
        cen.dropped.add((tile, wave, "neither"))


# ---- the tiles of a launch ------------------------------------------------------------------------------------------------------
def planned_tiles(lib, fmt, settings, address, total, first, num):
    """([(tile kind, first block, blocks it owns)], [launch kinds]) of the inverse transform's plan for blocks [first, first + num)"""
    out = (PlannedLaunch * 8)()
    n = lib.dxtlt_debug_plan_transform(FMT_ID[fmt], 1, settings[0], int(settings[1]), int(settings[2]), address, 0, total, first, num, out, 8)
    assert 0 < n <= 8, (fmt, settings, address, total, first, num, n)
    tiles, covered = [], 0
    for l in list(out)[:n]:
        T = l.threads * 16 // BLOCK[fmt]
        start = first + l.aos_offset // BLOCK[fmt]
        assert start == first + covered and l.aos_offset % BLOCK[fmt] == 0
        if l.kind == 0:
            assert l.range_blocks == l.workgroups * T
            tiles += [("aligned", start + i * T, T) for i in range(l.workgroups)]
        else:
            assert l.kind == 2 and T == TILE[fmt]
            rest = l.range_blocks - l.full_tiles * T
            assert 0 <= rest < T and l.workgroups == l.full_tiles + (1 if rest else 0)
            tiles += [("shifted", start + i * T, T) for i in range(l.full_tiles)]
            if rest:
                tiles.append(("edge", start + l.full_tiles * T, rest))
        covered += l.range_blocks
    assert covered == num
    return tiles, [l.kind for l in list(out)[:n]]


def run_tiles(cen, group, tiles, single):
    """every tile's lanes through the sink: `store` in a full tile, `store_edge` in the edge tile"""
    fmt = cen.case.fmt
    pv, W = PV[fmt], WAVE[fmt]
    for tile, start, own in tiles:
        if tile == "edge":
            wave, run = ("single", (group[0][0], group[0][1])) if single else ("edge", None)   # (no_wave_run: every lane looks)
            for t in range((own + pv - 1) // pv):                                              # (the lanes that hold a block)
                b, have = start + pv * t, min(pv, own - pv * t)
                if fmt in RGBA:
                    for j in range(have):
                        put_pixels(cen, group, tile, wave, "own", run, b + j)
                else:
                    put_channels(cen, group, tile, wave, run, b, have)
            continue
        assert own % W == 0
        for w0 in range(start, start + own, W):
            if single:
                wave, run = "single", (group[0][0], group[0][1])
            else:
                run = region_of_run(group, w0, W)
                wave = "uniform" if run is not None else "per lane"
            if fmt in RGBA:
                for b in range(w0, w0 + W):     # BC1: dealt out again, lane l has blocks l and 64 + l -- every block one store call
                    put_pixels(cen, group, tile, wave, "exchange" if fmt == "bc1" else "own", run, b)
            else:
                for lane in range(64):
                    put_channels(cen, group, tile, wave, run, w0 + pv * lane, pv)


def run_plain(cen, group, single):
    """the plain decoders over the group's range, 256 lanes a workgroup, 64 a wave"""
    case = cen.case
    fmt = case.fmt
    pv = 1 if fmt in RGBA else PV[fmt]         # (one block a lane for BC1 too: decode_image_kernel)
    W = 64 * pv
    tile = "plain vector" if case.in_off % BLOCK[fmt] == 0 else "plain bytes"
    first, end = group[0][1], group[-1][1] + group[-1][2]
    for w0 in range(first, end, W):
        if single:
            wave, run = "single", (group[0][0], group[0][1])
        else:
            run = region_of_run(group, w0, W)          # (the last wave's run may reach past the last region)
            wave = "uniform" if run is not None else "per lane"
        for lane in range(64):
            b = w0 + pv * lane
            if b >= end:
                break
            have = min(pv, end - b)
            if fmt in RGBA:
                put_pixels(cen, group, tile, wave, "own", run, b)
            else:
                put_channels(cen, group, tile, wave, run, b, have)


def census(lib, case):
    cen = Census(case)
    fmt, address = case.fmt, PLAN_ADDRESS + case.in_off
    single = case.entry in ("single", "plain single")
    if single:
        assert len(case.regions) == 1 and case.regions[0][1] and case.regions[0][2]
    if case.entry in ("plain single", "plain regions"):
        for group in groups_of(case.regions):
            run_plain(cen, group, single)
    elif case.entry in ("single", "regions"):
        for group in groups_of(case.regions):
            first, end = group[0][1], group[-1][1] + group[-1][2]
            tiles, kinds = planned_tiles(lib, fmt, case.settings, address, case.total, first, end - first)
            cen.kinds.append(kinds)
            run_tiles(cen, group, tiles, single)
    else:
        assert case.entry == "batch"
        for e in plan_batch(lib, [as_item(case)]):
            (group,) = groups_of(case.regions, e.first_region, e.region_count)
            first, end = group[0][1], group[-1][1] + group[-1][2]
            assert (e.first_block, e.range_blocks) == (first, end - first)
            if e.launch < 0:        # shifts off their element widths: the regions kernels, alone
                tiles, kinds = planned_tiles(lib, fmt, case.settings, address, case.total, first, end - first)
                cen.kinds.append(["alone"] + kinds)
            else:                   # tiles of 256 lanes whatever the form
                T = TILE[fmt]
                rest = e.range_blocks - e.full_tiles * T
                assert 0 <= rest < T and e.end_wg - e.first_wg == e.full_tiles + (1 if rest else 0)
                tiles = [("aligned" if e.form == 1 else "shifted", first + i * T, T) for i in range(e.full_tiles)]
                if rest:
                    tiles.append(("edge", first + e.full_tiles * T, rest))
                cen.kinds.append(["batch", e.form])
            run_tiles(cen, group, tiles, False)
    assert all(c is not None for c in cen.all_cells()), (case.name, "a block of a region is written by no lane")
    return cen


def cell_of_byte(case, cen, region, offset):
    """what a failure message says about byte `offset` of region `region`'s output"""
    _, width, height = case.regions[region]
    y, x = divmod(offset, case.pitches[region])
    x //= BPP[case.fmt]
    if x >= width or y >= height:
        return f"row {y}, byte {offset - y * case.pitches[region]} of the row: pitch padding, no block's"
    local = (y // 4) * ((width + 3) // 4) + x // 4
    return f"pixel ({x}, {y}), block {local} of the region = block {case.regions[region][0] + local} of the buffer: {cen.cells[region][local]}"
