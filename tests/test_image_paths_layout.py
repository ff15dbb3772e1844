"""Which store and lookup paths of the image decode sinks the device tests of tests/test_image_paths_gpu.py reach, proved on a
machine without a GPU (docs/IMAGE_DECODE.md, "What the tests reach").

build_cases lists the calls those tests make, as plain data.  tests/image_paths.py says which cell -- (tile kind, wave path, lane
path, store class, clip class), its docstring defines them -- every block of every case is in.  The test here computes that census
for the whole list and asserts, per entry point and format, that the union is EXACTLY the set of cells that can exist: thin the
list and a cell goes unreached; reach a cell that `why_not` calls impossible and the reasoning is wrong.  Every cell of the full
product is either in the literal LANES / TILE_WAVE below or has a reason in `why_not`, and that too is asserted.

The lists (T: blocks of a 256-lane tile, 512 for BC1 / BC4 and 256 otherwise; W: blocks of a wave, 128 / 64):

  (a) block-row length against the wave -- the single-image calls, fused and plain, default settings.  Every block-row length bw
      in 1 .. 130 at two block rows, width 4 bw - c and height 8 - r with c and r rotating so that each meets odd and even bw;
      bw in TALL again as an image of 2T + 9 blocks or more under each launch shape the plan has -- [2] (odd total_blocks:
      shifted tiles and an edge tile), [0, 2] (aligned tiles, an edge launch), [0] (aligned tiles only) and [2] with a range that
      ends on a tile: without the last two no full tile would ever hold an image's last block, its only corner block.
  (b) store class -- every (pointer, pitch) alignment of ALIGNMENTS x bw in 5, 6, 65, 66 clipped on both sides, under the same
      shapes; the plain calls with the block pointer on and off a multiple of the block size.
  (c) region boundary phase -- the regions calls, fused and plain, and the batch call.  Region 0 ends at block T + k for every k
      in 0 .. W - 1, inside a full tile; region 1 starts g = 0, 1, 2 blocks further and ends in the edge tile, where a gap and a
      small third region follow, so that BC4's split pairs occur in full tiles and in the edge tile; where T + k is no multiple of
      the block-row length a one-row region of (T + k) mod bw blocks leads.  Neighbouring regions have different store classes
      (image_paths.store_class, not merely different pointers), so a per-lane wave always meets a divergent store choice.
      Every table once with an odd total_blocks (shifted tiles) and once with a multiple of 128 (aligned tiles).  (c0): both
      boundaries ON wave ends, once per alignment -- the only way a region's last block row lies in a uniform wave.
  (d) seeded random region tables, 24 per format, for the regions call and the batch call: reported, not required to reach
      anything."""
import collections
import math

import numpy as np
import pytest

import image_paths
from image_batch_common import TILE, load
from image_paths import Case, WAVE, cell5, census
from image_regions_common import BPP, FMTS, blocks_of, default_settings, other_settings, region_end, settings_of

CLIPS = ("whole", "right", "bottom", "corner")
CLIPPED = ("right", "bottom", "corner")

# (pixel pointer modulo 16, what the pitch adds to a multiple of 16): the store class is image_paths.store_class of the pair
ALIGNMENTS = {
    "bc1": ((0, 0), (4, 0), (0, 4), (8, 8), (12, 12)),      # stream16, then plain16 four ways
    "bc2": ((0, 0), (4, 0), (0, 4), (8, 8), (12, 12)),
    "bc3": ((0, 0), (4, 0), (0, 4), (8, 8), (12, 12)),
    "bc5": ((0, 0), (4, 0), (0, 4), (8, 8), (12, 12), (2, 2)),                          # stream8, dwords x 2, plain8, dwords, halfwords
    "bc4": ((0, 0), (4, 0), (0, 4), (8, 8), (12, 12), (2, 2), (1, 1), (3, 3), (1, 0)),  # ... and bytes three ways
}
TALL = (5, 6, 63, 64, 65, 127, 128, 129, 130)
ENDS_ON_A_TILE = (5, 6, 64, 128)
SHAPES = {"[2]": [2], "[0, 2]": [0, 2], "[0]": [0], "[2] whole tiles": [2]}


def pitch_of(fmt, width, delta):
    return (BPP[fmt] * width + 15) // 16 * 16 + delta


def tall_shape(fmt, bw, shape):
    """(block rows, total_blocks) of an image of 2T + 9 blocks or more with `bw` blocks a row that the plan gives `shape`"""
    need = 2 * TILE[fmt] + 9
    if shape == "[2]":
        rows = -(-need // bw)
        return rows, bw * rows | 1
    if shape == "[0, 2]":
        rows = -(-need // bw)
        rows += 1 if bw * rows % 256 == 0 else 0
        return rows, (bw * rows + 127) // 128 * 128
    step = (256 if shape == "[0]" else TILE[fmt]) // math.gcd(bw, TILE[fmt])
    rows = -(-need // (bw * step)) * step
    return rows, bw * rows + (0 if shape == "[0]" else 1)


def image_case(entry, fmt, bw, rows, c, r, align, total, in_off, name):
    w, h = 4 * bw - c, 4 * rows - r
    return Case(entry, fmt, default_settings(fmt), in_off, total, [(0, w, h)], [align[0]], [pitch_of(fmt, w, align[1])], 0,
                f"{name} {entry} {fmt} {w}x{h} bw={bw} in+{in_off} out+{align[0]} pitch+{align[1]}")


def single_cases(lib, fmt):
    fused, plain = [], []
    # (a)
    for bw in range(1, 131):
        c, r = (bw // 2) % 4, (bw // 2 + bw // 8) % 4
        fused.append(image_case("single", fmt, bw, 2, c, r, (0, 0), 2 * bw, 0, "(a)"))
        plain.append(image_case("plain single", fmt, bw, 2, c, r, (0, 0), 2 * bw, 0, "(a)"))
    for bw in TALL:
        c, r = (bw // 2) % 4, (bw // 2 + bw // 8) % 4
        for shape in SHAPES:
            if shape in ("[0]", "[2] whole tiles") and bw not in ENDS_ON_A_TILE:
                continue
            rows, total = tall_shape(fmt, bw, shape)
            fused.append(image_case("single", fmt, bw, rows, c, r, (0, 0), total, 0, f"(a) {shape}"))
        rows, total = tall_shape(fmt, bw, "[2]")
        plain.append(image_case("plain single", fmt, bw, rows, c, r, (0, 0), total, 0, "(a) tall"))
    # (b)
    for i, align in enumerate(ALIGNMENTS[fmt]):
        for bw in (5, 6, 65, 66):
            c, r = 1 + (bw + i) % 3, 1 + (bw // 2 + i) % 3
            fused.append(image_case("single", fmt, bw, 2, c, r, align, 2 * bw, 0, "(b)"))
            for in_off in (0, 1):
                plain.append(image_case("plain single", fmt, bw, 2, c, r, align, 2 * bw, in_off, "(b)"))
            for shape in SHAPES:
                if shape in ("[0]", "[2] whole tiles") and bw not in ENDS_ON_A_TILE:
                    continue
                rows, total = tall_shape(fmt, bw, shape)
                fused.append(image_case("single", fmt, bw, rows, c, r, align, total, 0, f"(b) {shape}"))
            rows, total = tall_shape(fmt, bw, "[2]")
            plain.append(image_case("plain single", fmt, bw, rows, c, r, align, total, (i + bw) % 2, "(b) tall"))
            if bw in (5, 66):     # the transformed buffer off a 128-byte line: shifted tiles whatever total_blocks is
                in_off = 8 if bw == 5 else 16
                fused.append(image_case("single", fmt, bw, 2, c, r, align, 2 * bw + 4, in_off, "(b) residue"))
                fused.append(image_case("single", fmt, bw, rows, c, r, align, bw * rows + 6, in_off, "(b) residue tall"))
    # ask the plan, do not guess
    for case in fused:
        for shape, kinds in SHAPES.items():
            if f" {shape} single" in case.name:
                n = blocks_of(*case.regions[0][1:])
                tiles, got = image_paths.planned_tiles(lib, fmt, case.settings, image_paths.PLAN_ADDRESS, case.total, 0, n)
                assert got == kinds and (tiles[-1][0] == "edge") == (shape in ("[2]", "[0, 2]")), (case.name, got)
    return fused, plain


SMALL = ((1, 1), (3, 2), (5, 3), (9, 6), (4, 4), (2, 7))   # the third region of a (c) table: 1, 1, 2, 6, 1, 2 blocks


def aligns_by_class(fmt):
    """{store class: [alignments of ALIGNMENTS[fmt] that have it]}, in the order of their first appearance"""
    out = {}
    for a in ALIGNMENTS[fmt]:
        out.setdefault(image_paths.store_class(fmt, a[0], a[1]), []).append(a)
    return out


def align_of_class(fmt, index, pick):
    """an alignment of store class number `index` (modulo the number of classes), its ways taken in turn by `pick`"""
    ways = list(aligns_by_class(fmt).values())
    ways = ways[index % len(ways)]
    return ways[pick % len(ways)]


def other_class(fmt, index, step):
    """the number of a store class other than class `index`: every other one in turn as `step` grows"""
    nc = len(aligns_by_class(fmt))
    return (index + 1 + step % (nc - 1)) % nc


def boundary_table(fmt, k, variant):
    """(regions, alignments, total_blocks) of (c): region 0 ends at block T + k.  Neighbouring regions have different store
    CLASSES: region 0 takes the classes in turn with k -- for BC1 - BC3, which have two, the streaming side alternates -- region 1
    every other class in turn, the third region a class other than region 1's, the leading region one other than region 0's."""
    T = TILE[fmt]
    nc, bws, target = len(aligns_by_class(fmt)), (7, 8, 9), TILE[fmt] + k
    c0 = k % nc
    c1 = other_class(fmt, c0, k // nc)
    c2 = other_class(fmt, c1, k // 7)
    regions, aligns = [], []
    bw0 = next((b for b in (bws[(k + j) % 3] for j in range(3)) if target % b == 0), None)
    lead = 0
    if bw0 is None:   # a one-row region of `lead` blocks in front makes up the count
        bw0 = bws[k % 3]
        lead = target % bw0
        regions.append((0, 4 * lead - (1 + k % 3), 4 - (k // 3) % 4))
        aligns.append(align_of_class(fmt, other_class(fmt, c0, k // 5), k // 3))
    regions.append((lead, 4 * bw0 - (1 + k % 3), 4 * ((target - lead) // bw0) - (1 + (k // 3) % 3)))
    aligns.append(align_of_class(fmt, c0, k // nc))
    assert region_end(regions[-1]) == target
    gap = (k // 2) % 3
    bw1 = bws[(k + 1) % 3]
    rows1 = -(-(T - k - gap + 10) // bw1)
    regions.append((target + gap, 4 * bw1 - (1 + (k + 1) % 3), 4 * rows1 - (1 + (k // 2 + 1) % 3)))
    aligns.append(align_of_class(fmt, c1, k // 2))
    end1 = region_end(regions[-1])
    assert 2 * T + 10 <= end1 < 2 * T + 19
    regions.append((end1 + (k + k // 3) % 3,) + SMALL[k % 6])
    aligns.append(align_of_class(fmt, c2, k // 3))
    end = region_end(regions[-1]) + k % 3
    assert end < 3 * T
    return regions, aligns, (end | 1 if variant == "shifted" else (end + 127) // 128 * 128)


def wave_end_table(fmt, i, variant):
    """(c0): regions of T, T and 10 blocks side by side, their boundaries on wave ends; region 0 has alignment i, its neighbour
    another class, the third region another class again"""
    T, B = TILE[fmt], ALIGNMENTS[fmt]
    c, r = 1 + i % 3, 1 + (i // 3) % 3
    regions = [(0, 32 - c, T // 2 - r), (T, 32 - (4 - c), T // 2 - (4 - r)), (2 * T, 20 - c, 8 - r)]
    c0 = list(aligns_by_class(fmt)).index(image_paths.store_class(fmt, B[i][0], B[i][1]))
    c1 = other_class(fmt, c0, i)
    aligns = [B[i], align_of_class(fmt, c1, i), align_of_class(fmt, other_class(fmt, c1, i // 2), i // 2)]
    end = 2 * T + 10
    return regions, aligns, (end | 1 if variant == "shifted" else (end + 127) // 128 * 128)


def table_case(entry, fmt, settings, in_off, regions, aligns, total, seed, name):
    return Case(entry, fmt, settings, in_off, total, list(regions), [a[0] for a in aligns],
                [pitch_of(fmt, w, a[1]) for (_, w, _), a in zip(regions, aligns)], seed, f"{name} {entry} {fmt} in+{in_off} total={total}")


def region_cases(fmt):
    fused, plain, batch = [], [], []
    for variant in ("shifted", "aligned"):
        tables = [(f"(c) k={k} {variant}", default_settings(fmt) if k % 4 else other_settings(fmt)) + boundary_table(fmt, k, variant)
                  for k in range(WAVE[fmt])]
        tables += [(f"(c0) {i} {variant}", default_settings(fmt)) + wave_end_table(fmt, i, variant) for i in range(len(ALIGNMENTS[fmt]))]
        for name, settings, regions, aligns, total in tables:
            fused.append(table_case("regions", fmt, settings, 0, regions, aligns, total, 0, name))
            # the plain decoders have no plan: the second pass runs them with the block pointer off the block size
            plain.append(table_case("plain regions", fmt, settings, 0 if variant == "shifted" else 1, regions, aligns, total, 0, name))
            batch.append(table_case("batch", fmt, settings, 0, regions, aligns, total, 0, name))
    # one item per format at a buffer address = 1 (mod 8): its shifts are off the element widths and it goes out alone
    for k, in_off in ((5, 1), (6, 9)):
        regions, aligns, total = boundary_table(fmt, k, "shifted")
        batch.append(table_case("batch", fmt, default_settings(fmt), in_off, regions, aligns, total, 0, f"(c) k={k} alone"))
    return fused, plain, batch


RANDOM_TABLES = 24


def random_cases(fmt):
    fused, batch = [], []
    B = ALIGNMENTS[fmt]
    for n in range(RANDOM_TABLES):
        rng = np.random.default_rng(0x1A6E0000 + 1000 * FMTS.index(fmt) + n)
        regions, aligns, at = [], [], int(rng.integers(0, 6))
        for _ in range(int(rng.integers(1, 41))):
            if rng.integers(0, 8) == 0:     # a zero-size region, anywhere
                regions.append((int(rng.integers(0, 2**40)), 0, int(rng.integers(0, 9))) if rng.integers(0, 2) else (at, 5, 0))
                aligns.append((0, 0))
                continue
            w, h = int(rng.integers(1, 71)), int(rng.integers(1, 71))
            regions.append((at, w, h))
            aligns.append(B[int(rng.integers(0, len(B)))])
            at = region_end(regions[-1]) + int(rng.integers(0, 6))
        if all(w == 0 or h == 0 for _, w, h in regions):
            regions.append((at, 9, 9))
            aligns.append(B[0])
            at = region_end(regions[-1])
        in_off = (0, 1, 8, 16)[int(rng.integers(0, 4))]
        combos = settings_of(fmt)
        settings = combos[int(rng.integers(0, len(combos)))]
        total = at + int(rng.integers(0, 4))
        fused.append(table_case("regions", fmt, settings, in_off, regions, aligns, total, 1, f"(d) table {n}"))
        batch.append(table_case("batch", fmt, settings, in_off, regions, aligns, total, 1, f"(d) table {n}"))
    return fused, batch


_CASES = {}


def build_cases(lib):
    """{list name: {format: [Case]}} -- "single", "plain single", "regions", "plain regions", "batch" carry the proof;
    "random regions" and "random batch" are (d)"""
    if not _CASES:
        out = collections.defaultdict(dict)
        for fmt in FMTS:
            out["single"][fmt], out["plain single"][fmt] = single_cases(lib, fmt)
            out["regions"][fmt], out["plain regions"][fmt], out["batch"][fmt] = region_cases(fmt)
            out["random regions"][fmt], out["random batch"][fmt] = random_cases(fmt)
        _CASES.update(out)
    return _CASES


_CENSUS = {}


def census_of(lib, case):
    """computed once per case and shared"""
    if case.name not in _CENSUS:
        _CENSUS[case.name] = (case, census(lib, case))
    assert _CENSUS[case.name][0] == case, ("two cases share a name", case.name)
    return _CENSUS[case.name][1]


# ---- the cells that can exist -------------------------------------------------------------------------------------------------
TILES = ("aligned", "shifted", "edge", "plain vector", "plain bytes")
WAVES = ("single", "uniform", "per lane", "edge")
REGION_TILE_WAVE = {("aligned", "uniform"), ("aligned", "per lane"), ("shifted", "uniform"), ("shifted", "per lane"), ("edge", "edge")}
TILE_WAVE = {
    "single": {("aligned", "single"), ("shifted", "single"), ("edge", "single")},
    "plain single": {("plain vector", "single"), ("plain bytes", "single")},
    "regions": REGION_TILE_WAVE,
    "plain regions": {("plain vector", "uniform"), ("plain vector", "per lane"), ("plain bytes", "uniform"), ("plain bytes", "per lane")},
    "batch": REGION_TILE_WAVE,
}
STORES = {"bc1": ("stream16", "plain16"), "bc2": ("stream16", "plain16"), "bc3": ("stream16", "plain16"),
          "bc4": ("stream8", "plain8", "dwords", "halfwords", "bytes"), "bc5": ("stream8", "plain8", "dwords", "halfwords", "bytes")}
LANE_PATHS = {"bc1": ("exchange", "own"), "bc2": ("exchange", "own"), "bc3": ("exchange", "own"), "bc4": ("rows8", "alone"),
              "bc5": ("rows8", "alone")}
# (lane path, store class, clip class) of one block, in whatever tile and wave that has the lane path
LANES = {
    "bc1": {(lane, s, c) for lane in ("exchange", "own") for s in ("stream16", "plain16") for c in CLIPS},
    "bc2": {("own", s, c) for s in ("stream16", "plain16") for c in CLIPS},
    "bc3": {("own", s, c) for s in ("stream16", "plain16") for c in CLIPS},
    # BC4: a whole block is alone under ANY alignment -- an odd block column, a pair that straddles a block-row end, a pair split
    # between regions
    "bc4": {("rows8", "stream8", "whole"), ("rows8", "plain8", "whole")}
           | {("alone", s, c) for s in ("stream8", "plain8", "dwords", "halfwords", "bytes") for c in CLIPS},
    "bc5": {("rows8", "stream8", "whole"), ("rows8", "plain8", "whole")}
           | {("alone", s, c) for s in ("dwords", "halfwords") for c in CLIPS}
           | {("alone", s, c) for s in ("stream8", "plain8") for c in CLIPPED},
}


def why_not(entry, fmt, cell):
    """the reason a cell of the full product cannot occur, or None"""
    tile, wave, lane, store, clip = cell
    plain_entry, plain_tile = entry.startswith("plain"), tile.startswith("plain")
    if plain_entry != plain_tile:
        return "the fused calls run tiles, the plain calls the plain decoders"
    if (wave == "single") != (entry in ("single", "plain single")):
        return "the single-image kernels have no lookup, the region kernels always have one"
    if wave != "single" and (tile == "edge") != (wave == "edge"):
        return "the edge tile never asks for the wave's run (no_wave_run), every other wave does"
    if lane == "exchange" and not (fmt == "bc1" and tile in ("aligned", "shifted")):
        return "only BC1 has two blocks a lane to deal out again, and store_edge and the plain decoders keep a lane's own blocks"
    if lane == "own" and fmt == "bc1" and tile in ("aligned", "shifted"):
        return "a BC1 full tile always exchanges"
    if fmt == "bc5" and store == "bytes":
        return "the C ABI refuses a two-byte pixel at an odd address or pitch"
    if lane == "rows8" and clip != "whole":
        return "rows8 needs the lane's blocks whole: 4 (bx + PV) <= width and rows == 4"
    if lane == "rows8" and store not in ("stream8", "plain8"):
        return "rows8 needs the pixel pointer and the pitch multiples of 8"
    if fmt == "bc5" and lane == "alone" and clip == "whole" and store in ("stream8", "plain8"):
        return "a whole BC5 block is a lane's whole vector: on 8-byte rows it always takes rows8"
    return None


def reachable(entry, fmt):
    return {(tile, wave) + lane for tile, wave in TILE_WAVE[entry] for lane in LANES[fmt]
            if (lane[0] == "exchange") == (fmt == "bc1" and tile in ("aligned", "shifted"))}


def pairs_expected(tile, wave):
    """what can become of a BC4 lane's two blocks"""
    if wave == "uniform":      # the run lies in one region, and so does every pair; a range's odd last block ends the last region,
        return {"same region"}  # so the run of its wave reaches past it and is no uniform one
    if wave == "single":       # a full tile's lanes all hold two blocks; the last lane of an odd image holds one
        return {"same region"} | ({"first only"} if tile in ("edge", "plain vector", "plain bytes") else set())
    return {"same region", "two regions", "first only", "second only", "neither"}


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


PROOF_LISTS = ("single", "plain single", "regions", "plain regions", "batch")


@pytest.mark.parametrize("fmt", FMTS)
def test_every_excluded_cell_has_a_reason(fmt):
    for entry in PROOF_LISTS:
        can = reachable(entry, fmt)
        for tile in TILES:
            for wave in WAVES:
                for lane in LANE_PATHS[fmt]:
                    for store in STORES[fmt]:
                        for clip in CLIPS:
                            cell = (tile, wave, lane, store, clip)
                            assert (cell in can) != (why_not(entry, fmt, cell) is not None), (entry, fmt, cell, why_not(entry, fmt, cell))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("entry", PROOF_LISTS)
def test_the_case_lists_reach_every_cell_that_can_exist(lib, entry, fmt):
    cases = build_cases(lib)[entry][fmt]
    reached, pairs, dropped = set(), collections.defaultdict(lambda: collections.defaultdict(set)), set()
    alone = 0
    for case in cases:
        cen = census_of(lib, case)
        alone += any(k[0] == "alone" for k in cen.kinds)
        dropped |= cen.dropped
        for cell in cen.all_cells():
            reached.add(cell5(cell))
            if cell.pair is not None:
                pairs[(cell.tile, cell.wave)][cell.pair].add((cell.slot, cell.store))
                assert cell.lane == "alone" or cell.pair == "same region", (case.name, cell)   # rows8 is for two blocks of one region
    can = reachable(entry, fmt)
    for cell in sorted(reached - can):
        pytest.fail(f"{entry} {fmt}: reached {cell}, which cannot occur: {why_not(entry, fmt, cell)}")
    assert not can - reached, (entry, fmt, "unreached cells", sorted(can - reached))
    # a uniform wave holds no gap block, and a single image has no gap
    assert all(wave in ("per lane", "edge") for _, wave, _ in dropped), dropped
    if entry == "batch":
        assert alone >= 2, "no item went out alone"
    if fmt == "bc4":
        for tile, wave in sorted(TILE_WAVE[entry]):
            got = dict(pairs[(tile, wave)])
            if (tile, wave, "neither") in dropped:
                got["neither"] = set()
            assert set(got) == pairs_expected(tile, wave), (entry, tile, wave, sorted(got))
            # a split pair under two alignments or more: counted for the first and for the second block of the pair apart, since
            # the two blocks of a "two regions" pair lie in images of different classes anyway
            for state, slots in (("two regions", (0, 1)), ("first only", (0,)), ("second only", (1,))):
                if state in got and wave != "single":
                    for slot in slots:
                        assert len({s for sl, s in got[state] if sl == slot}) >= 2, (entry, tile, wave, state, slot, got[state])
    elif entry in ("regions", "plain regions", "batch"):
        assert {(t, w) for t, w, _ in dropped} == {tw for tw in TILE_WAVE[entry] if tw[1] != "uniform"}, dropped


@pytest.mark.parametrize("fmt", FMTS)
def test_the_geometry_of_the_lists(lib, fmt):
    """what the lists promise about block-row lengths, phases and store classes, whatever the census says"""
    cases = build_cases(lib)
    for entry in ("single", "plain single"):
        small = [c for c in cases[entry][fmt] if c.name.startswith("(a)") and c.regions[0][2] <= 8]
        bws = collections.defaultdict(set)
        for c in small:
            _, w, h = c.regions[0]
            bws[(w + 3) // 4].add(((-w) % 4, 8 - h))
        assert sorted(bws) == list(range(1, 131))
        for parity in (0, 1):
            assert {c for bw, s in bws.items() if bw % 2 == parity for c, _ in s} == {0, 1, 2, 3}
            assert {r for bw, s in bws.items() if bw % 2 == parity for _, r in s} == {0, 1, 2, 3}
    tall = [c for c in cases["single"][fmt] if c.name.startswith("(a) [")]
    assert all(blocks_of(*c.regions[0][1:]) >= 2 * TILE[fmt] + 9 for c in tall)
    assert {(c.regions[0][1] + 3) // 4 for c in tall if "[0, 2]" in c.name} == set(TALL)
    for entry in ("regions", "plain regions", "batch"):
        phases, before, behind, orders = collections.defaultdict(set), set(), set(), set()
        for c in cases[entry][fmt]:
            if not c.name.startswith("(c) ") or "alone" in c.name:
                continue
            k = int(c.name.split("k=")[1].split()[0])
            boundary = next(i for i, r in enumerate(c.regions) if region_end(r) == TILE[fmt] + k)
            first1 = c.regions[boundary + 1][0]
            phases[c.name.split()[2]].add(k)
            assert first1 - (TILE[fmt] + k) in (0, 1, 2) and region_end(c.regions[boundary + 1]) > 2 * TILE[fmt]
            classes = [image_paths.store_class(fmt, o, p) for o, p in zip(c.out_offs, c.pitches)]
            assert all(a != b for a, b in zip(classes, classes[1:])), (c.name, classes, "neighbouring regions share a store class")
            orders.add((classes[boundary] == "stream16", classes[boundary + 1] == "stream16"))
            for (_, w, h) in c.regions[boundary:boundary + 2]:
                assert w % 4 and h % 4, (c.name, "both regions are clipped on both sides")
            before.add(image_paths.store_class(fmt, c.out_offs[boundary], c.pitches[boundary]))
            behind.add(image_paths.store_class(fmt, c.out_offs[boundary + 1], c.pitches[boundary + 1]))
        assert before == behind == {image_paths.store_class(fmt, o, d) for o, d in ALIGNMENTS[fmt]} and len(before) == len(STORES[fmt]) - (fmt == "bc5")
        if fmt in image_paths.RGBA:     # two classes: the streaming image on either side of the boundary
            assert orders == {(True, False), (False, True)}
        for c in cases[entry][fmt]:
            if c.name.startswith("(c0)"):
                classes = [image_paths.store_class(fmt, o, p) for o, p in zip(c.out_offs, c.pitches)]
                assert all(a != b for a, b in zip(classes, classes[1:])), (c.name, classes)
        assert phases == {"shifted": set(range(WAVE[fmt])), "aligned": set(range(WAVE[fmt]))}


def test_the_random_tables_report(lib):
    """(d): what the random tables reach is printed (pytest -rA), and nothing they reach may be a cell that cannot occur"""
    cases = build_cases(lib)
    lines = []
    for name, entry in (("random regions", "regions"), ("random batch", "batch")):
        for fmt in FMTS:
            reached = set()
            assert len(cases[name][fmt]) == RANDOM_TABLES
            for case in cases[name][fmt]:
                assert 1 <= len(case.regions) <= 41
                reached |= {cell5(c) for c in census_of(lib, case).all_cells()}
            can = reachable(entry, fmt)
            assert reached <= can, (name, fmt, sorted(reached - can))
            lines.append(f"{name} {fmt}: {len(reached)} of {len(can)} cells; not reached: {sorted(can - reached)}")
    print("\n".join(lines))
