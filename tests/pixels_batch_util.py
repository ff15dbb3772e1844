"""What the tests of the batched pixel calls share (include/dxtlt_pixels.h: dxtlt_transform_pixels_batch_device,
dxtlt_transform_pixels_batch_auto_device): the C structures, the case lists of the GPU tests -- built here so that the no-device
test can count what they reach -- and one-arena buffers with guard bytes for the GPU tests."""
from __future__ import annotations

import ctypes as C

import numpy as np

import pixels_ref

GUARD = 256
TILE = 4096
WINDOW = 32768
LINE = 128
COUNTS = [1, 15, 16, 17, 4095, 4096, 4097, 8193, 87381]
AUTO_COUNTS = [1, 17, 4097, 32768 + 7, 87381]
CLASSES = [(B, inv, dec, lay) for B in (4, 3) for inv in (0, 1) for dec in (0, 1) for lay in (0, 1, 2)]


class Item(C.Structure):                      # DxtltPixelBatchItem
    _fields_ = [("d_input", C.c_void_p), ("d_output", C.c_void_p), ("len", C.c_uint64), ("pixel_bytes", C.c_uint8),
                ("inverse", C.c_uint8), ("decorrelate", C.c_uint8), ("layout", C.c_uint8), ("reserved", C.c_uint8 * 4)]


class AutoItem(C.Structure):                  # DxtltPixelBatchAutoItem
    _fields_ = [("d_input", C.c_void_p), ("d_output", C.c_void_p), ("len", C.c_uint64), ("pixel_bytes", C.c_uint8),
                ("decorrelate", C.c_uint8), ("layout", C.c_uint8), ("reserved", C.c_uint8 * 5)]


class Launch(C.Structure):                    # DxtltDebugPixelBatchLaunch
    _fields_ = [("pixel_bytes", C.c_uint8), ("inverse", C.c_uint8), ("decorrelate", C.c_uint8), ("layout", C.c_uint8),
                ("items", C.c_uint32), ("workgroups", C.c_uint32), ("wide", C.c_uint32), ("table_offset", C.c_uint64),
                ("table_bytes", C.c_uint64)]


class Section(C.Structure):                   # DxtltDebugPixelBatchAutoSection
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint64), ("counter", C.c_uint32), ("in_arena", C.c_uint32)]


class PlanItem(C.Structure):                  # DxtltDebugPixelBatchAutoPlanItem
    _fields_ = [("chunk", C.c_uint32), ("reserved", C.c_uint32), ("arena_offset", C.c_uint64), ("arena_bytes", C.c_uint64),
                ("sections", Section * 6)]


class PlanChunk(C.Structure):                 # DxtltDebugPixelBatchAutoPlanChunk
    _fields_ = [("first_item", C.c_uint64), ("item_count", C.c_uint64), ("arena_bytes", C.c_uint64),
                ("candidate_launches", C.c_uint32), ("estimator_workgroups", C.c_uint32)]


def load(pkg):
    """the library with every symbol these tests call declared: a missing symbol raises AttributeError here, a failure"""
    l = pixels_ref.declare(C.CDLL(pkg._lib.lib_path()))
    vp, sz, i32, u64p = C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_uint64)
    l.dxtlt_transform_pixels_batch_device.argtypes, l.dxtlt_transform_pixels_batch_device.restype = [C.POINTER(Item), sz, vp], i32
    l.dxtlt_debug_plan_pixels_batch.argtypes = [C.POINTER(Item), sz, C.POINTER(Launch), sz, u64p]
    l.dxtlt_debug_plan_pixels_batch.restype = i32
    l.dxtlt_transform_pixels_batch_auto_device.argtypes = [C.POINTER(AutoItem), sz, vp]
    l.dxtlt_transform_pixels_batch_auto_device.restype = i32
    l.dxtlt_debug_plan_pixels_batch_auto.argtypes = [C.POINTER(AutoItem), sz, C.POINTER(PlanItem), C.POINTER(PlanChunk), sz, C.POINTER(sz)]
    l.dxtlt_debug_plan_pixels_batch_auto.restype = i32
    l.dxtlt_debug_pixels_batch_auto_last.argtypes, l.dxtlt_debug_pixels_batch_auto_last.restype = [u64p], None
    l.dxtlt_debug_pixels_batch_auto_last_totals.argtypes = [sz, u64p, i32]
    l.dxtlt_debug_pixels_batch_auto_last_totals.restype = i32
    l.dxtlt_debug_batch_auto_arena_cap.argtypes, l.dxtlt_debug_batch_auto_arena_cap.restype = [C.c_uint64], None
    l.dxtlt_debug_auto_last_estimation.argtypes, l.dxtlt_debug_auto_last_estimation.restype = [u64p, u64p], None
    l.dxtlt_transform_pixels_auto_device.argtypes = [vp, vp, sz, i32, vp, C.POINTER(C.c_bool), C.POINTER(C.c_uint8)]
    l.dxtlt_transform_pixels_auto_device.restype = i32
    l.dxtlt_debug_pixels_auto_last_totals.argtypes, l.dxtlt_debug_pixels_auto_last_totals.restype = [u64p, i32], i32
    l.dxtlt_debug_pixels_auto_candidates_into_device.argtypes = [vp, sz, i32, vp, vp]
    l.dxtlt_debug_pixels_auto_candidates_into_device.restype = i32
    l.dxtlt_debug_pixels_batch_candidates_device.argtypes = [C.POINTER(AutoItem), sz, sz, vp, C.c_uint64, vp]
    l.dxtlt_debug_pixels_batch_candidates_device.restype = i32
    l.dxtlt_last_error.restype = C.c_char_p
    return l


# ---- the case lists of tests/test_pixels_batch_gpu.py: (pixels, B, inverse, decorrelate, layout, input residue, output residue) ----
def cases_every_class():
    """all 24 classes, two items each, the pixel counts of COUNTS in turn"""
    out = []
    for k, (B, inv, dec, lay) in enumerate(CLASSES):
        for j in range(2):
            n = 2 * k + j
            out.append((COUNTS[n % len(COUNTS)], B, inv, dec, lay, (7 * n) % LINE, (11 * n + 3) % LINE))
    return out


def cases_wide_lookup():
    """one class, 300 items of 1-3 tiles: more than 255 entries begin inside one span of 4096 workgroups -- the wide index -- and
    most workgroups find their entry by bisection"""
    counts = [100, TILE, TILE + 1, 2 * TILE, 2 * TILE + 5, 3 * TILE - 1, 3 * TILE]
    return [(counts[k % len(counts)], 4, 0, 1, 2, (5 * k) % LINE, (3 * k) % LINE) for k in range(300)]


def cases_long_entries():
    """one class, items of 64, 65 and 130 tiles between one-tile items: workgroups whose first fetched entry already owns them"""
    counts = [10, 64 * TILE, 77, 65 * TILE - 1, TILE, 130 * TILE - 4095, 4000]
    return [(p, 4, 1, 1, 2, (9 * k) % LINE, (13 * k + 1) % LINE) for k, p in enumerate(counts)]


def cases_count(n):
    """batches of 1, 2, 64 and 65 items of one class"""
    return [(TILE + 1 + k, 3, 0, 0, 1, k % LINE, (2 * k) % LINE) for k in range(n)]


def cases_alignment(B, inverse):
    """128 items of 4097 pixels, (decorrelate, PLANAR_DELTA): d_input at residue k, d_output at residue 37 k mod 128 of a line"""
    return [(TILE + 1, B, inverse, 1, 2, k, (37 * k) % LINE) for k in range(LINE)]


def cases_mix(seed=0x51CE, n=40):
    """a seeded mix over all classes, counts and residues"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        B, inv, dec, lay = CLASSES[int(rng.integers(0, len(CLASSES)))] if k >= len(CLASSES) else CLASSES[k]
        out.append((COUNTS[int(rng.integers(0, len(COUNTS)))], B, inv, dec, lay, int(rng.integers(0, LINE)), int(rng.integers(0, LINE))))
    return out


def lookup_arms(cases):
    """per class of `cases`: (workgroups whose index entry owns them, workgroups that go through the bisection), by the rule of
    csrc/batch_lookup.h: the index names the owner of workgroup 64 * (wg // 64)"""
    arms = {}
    for cls in sorted({c[1:5] for c in cases}):
        ends, wg = [], 0
        for c in cases:
            if c[1:5] == cls and c[0]:
                wg += -(-c[0] // TILE)
                ends.append(wg)
        owner_of = np.searchsorted(np.array(ends), np.arange(wg), side="right")
        direct = int(sum(owner_of[w] == owner_of[64 * (w // 64)] for w in range(wg)))
        arms[cls] = (direct, wg - direct)
    return arms


# ---- one arena per side, every buffer between guard bytes ----------------------------------------------------------------------
def place(lengths, residues):
    """offsets of buffers of `lengths` bytes inside one arena whose base is on a LINE boundary: GUARD bytes at least in front of
    each, behind the last, buffer k at residue residues[k] of a line; (offsets, arena size)"""
    at, offs = 0, []
    for n, r in zip(lengths, residues):
        at += GUARD
        at += (r - at) % LINE
        offs.append(at)
        at += n
    return offs, at + GUARD


def source_bytes(cases, seed=1):
    """per case (input bytes, expected output bytes): forward items transform random pixels, inverse items take the transformed
    side of random pixels and restore them"""
    rng = np.random.default_rng(seed)
    pairs = []
    for P, B, inv, dec, lay, _ri, _ro in cases:
        px = rng.integers(0, 256, P * B, dtype=np.uint8)
        # a smooth half, so that deltas and subtract-green see small and wrapping values alike
        px[: P * B // 2] = (np.arange(P * B // 2) // 7 + rng.integers(0, 3, P * B // 2)).astype(np.uint8)
        t = pixels_ref.forward(px, B, bool(dec), lay)
        pairs.append((t, px) if inv else (px, t))
    return pairs


class Arenas:
    """the inputs of a batch in one device arena (fill 0x11) and its outputs in another (fill 0xEE), each buffer at its residue
    between GUARD bytes; check() compares every guard, gap and input byte and returns the outputs"""

    def __init__(self, dev, inputs, in_res, out_res, out_lengths=None):
        import torch

        self.lengths = [int(a.size) for a in inputs]
        self.out_lengths = self.lengths if out_lengths is None else out_lengths
        self.in_off, in_size = place(self.lengths, in_res)
        self.out_off, out_size = place(self.out_lengths, out_res)
        host = np.full(in_size, 0x11, dtype=np.uint8)
        for a, o in zip(inputs, self.in_off):
            host[o:o + a.size] = a
        self.src = torch.from_numpy(host).to(dev)
        self.src_before = self.src.clone()
        self.dst = torch.full((out_size,), 0xEE, dtype=torch.uint8, device=dev)
        assert self.src.data_ptr() % LINE == 0 and self.dst.data_ptr() % LINE == 0
        self.owned = np.zeros(out_size, dtype=bool)
        for n, o in zip(self.out_lengths, self.out_off):
            assert not self.owned[o:o + n].any()
            self.owned[o:o + n] = True

    def in_ptr(self, k):
        return self.src.data_ptr() + self.in_off[k]

    def out_ptr(self, k):
        return self.dst.data_ptr() + self.out_off[k]

    def check(self, written=None):
        """after a synchronize: guards and gaps untouched, inputs untouched; returns the output arena on the host.  written: the
        items whose outputs the call may have written (default all); the others must still hold the fill"""
        import torch

        torch.cuda.synchronize()
        host = self.dst.cpu().numpy()
        assert (host[~self.owned] == 0xEE).all(), "guard or gap bytes written"
        assert torch.equal(self.src, self.src_before), "input written"
        if written is not None:
            for k, (n, o) in enumerate(zip(self.out_lengths, self.out_off)):
                if k not in written:
                    assert (host[o:o + n] == 0xEE).all(), k
        return host

    def output(self, host, k):
        return host[self.out_off[k]:self.out_off[k] + self.out_lengths[k]]


def make_items(cases, arenas):
    arr = (Item * max(1, len(cases)))()
    for k, (P, B, inv, dec, lay, _ri, _ro) in enumerate(cases):
        n = P * B
        arr[k].d_input, arr[k].d_output, arr[k].len = (arenas.in_ptr(k) if n else None), (arenas.out_ptr(k) if n else None), n
        arr[k].pixel_bytes, arr[k].inverse, arr[k].decorrelate, arr[k].layout = B, inv, dec, lay
    return arr


def fake_items(cases, base=0x7000_0000_0000):
    """the cases as items at made-up addresses with the cases' residues (the plan hooks dereference nothing)"""
    lengths = [c[0] * c[1] for c in cases]
    in_off, in_size = place(lengths, [c[5] for c in cases])
    out_off, _ = place(lengths, [c[6] for c in cases])
    out_base = base + ((in_size + 4095) & ~4095) + (1 << 20)
    arr = (Item * max(1, len(cases)))()
    for k, (P, B, inv, dec, lay, _ri, _ro) in enumerate(cases):
        arr[k].d_input, arr[k].d_output, arr[k].len = base + in_off[k], out_base + out_off[k], lengths[k]
        arr[k].pixel_bytes, arr[k].inverse, arr[k].decorrelate, arr[k].layout = B, inv, dec, lay
    return arr


def plan(lib, arr, count, cap=64):
    """(return value, launches, table bytes) of dxtlt_debug_plan_pixels_batch"""
    out = (Launch * cap)()
    tb = C.c_uint64(77)
    n = lib.dxtlt_debug_plan_pixels_batch(arr, count, out, cap, C.byref(tb))
    return n, list(out[:max(0, min(n, cap))]), tb.value


# ---- the fused candidate kernels: tests/test_pixels_candidates_gpu.py ------------------------------------------------------------------
# Cases keep the tuple form above -- (pixels, B, 0, 0, 0, input residue, output residue) -- so that source_bytes, Arenas, fake_items and
# lookup_arms take them: a candidate launch is one class per pixel size.
ARENA_FILL = 0xEE
CANDIDATE_COUNTS = [1, 15, 16, 17, 4095, 4096, 4097, 8193, 12287]      # the single kernel
CANDIDATE_BATCH_COUNTS = [1, 17, 4096, 4097, 8193, 12287]
CANDIDATE_RESIDUES = [0, 1, 8, 15]
LONG_ITEM = 64 * TILE + 1
CANDIDATE_CHUNK_CAP = 600_000        # test_forced_chunks: the mixed batch in seven chunks


def candidate_case(pixels, B, in_res, k=0):
    return (pixels, B, 0, 0, 0, in_res, (3 * k + in_res) % LINE)


def cases_candidates_mixed():
    """40 items, the pixel sizes mixed: every count of CANDIDATE_BATCH_COUNTS and every input residue with both sizes, an empty item in
    the middle, and one item of 64 tiles and a pixel between one-tile items of its own size (both lookup arms of csrc/batch_lookup.h)"""
    out = [candidate_case(CANDIDATE_BATCH_COUNTS[k % 6], (4, 3)[(k + k // 6) % 2], CANDIDATE_RESIDUES[(k + k // 4) % 4], k) for k in range(36)]
    out[18:18] = [candidate_case(0, 4, 0, 36)]
    out[9:9] = [candidate_case(17, 4, 8, 37), candidate_case(LONG_ITEM, 4, 1, 38), candidate_case(1, 4, 15, 39)]
    return out


def cases_candidates_wide():
    """300 items of one to three tiles of 3-byte pixels, the counts of cases_wide_lookup: the wide index in ONE candidate launch"""
    return [candidate_case(c[0], 3, CANDIDATE_RESIDUES[k % 4], k) for k, c in enumerate(cases_wide_lookup())]


def last_lane_valid(pixels):
    """`valid` of the last lane with a pixel in the buffer's last tile (DXTLT_PIXEL_CANDIDATES_TILE): 16 = the vector arm of plane_store"""
    n = (pixels - 1) % TILE + 1
    return (n - 1) % 16 + 1


def candidates_of(flat, B):
    """the statement of a candidate arena or slice: candidates 0..4 of entropy_ref.CANDIDATES side by side, 5 * len bytes"""
    import entropy_ref

    return np.concatenate([pixels_ref.forward(flat, B, d, l) for d, l in entropy_ref.CANDIDATES[:5]])


def arena_differences(got, placed, fill=ARENA_FILL):
    """THE comparison of the candidate tests.  placed: [(offset, expected bytes, tag)], disjoint.  [] when every range of `got`
    equals its expectation and every other byte holds `fill`; else one line per range that differs and one for the strays."""
    image, covered = np.full(got.size, fill, dtype=np.uint8), np.zeros(got.size, dtype=bool)
    for off, want, tag in placed:
        assert 0 <= off and off + want.size <= got.size and not covered[off:off + want.size].any(), tag
        image[off:off + want.size] = want
        covered[off:off + want.size] = True
    if np.array_equal(got, image):
        return []
    out = []
    for off, want, tag in placed:
        bad = np.nonzero(got[off:off + want.size] != want)[0]
        if bad.size:
            i = int(bad[0])
            out.append(f"{tag}: {bad.size} of {want.size} bytes differ, first at byte {i} (got {int(got[off + i])}, want {int(want[i])})")
    stray = np.nonzero((got != fill) & ~covered)[0]
    if stray.size:
        out.append(f"{stray.size} bytes outside every slice were written, first at {int(stray[0])}")
    return out


def make_auto_items(cases, arenas):
    arr = (AutoItem * max(1, len(cases)))()
    for k, c in enumerate(cases):
        n = c[0] * c[1]
        arr[k].d_input, arr[k].d_output, arr[k].len = (arenas.in_ptr(k) if n else None), (arenas.out_ptr(k) if n else None), n
        arr[k].pixel_bytes, arr[k].decorrelate, arr[k].layout = c[1], 0xEE, 0xEE
    return arr


def fake_auto_items(cases):
    """the cases as auto items at made-up addresses with the cases' residues (the plan hook dereferences nothing)"""
    fake = fake_items(cases)
    arr = (AutoItem * max(1, len(cases)))()
    for k, c in enumerate(cases):
        arr[k].d_input, arr[k].d_output, arr[k].len, arr[k].pixel_bytes = fake[k].d_input, fake[k].d_output, fake[k].len, c[1]
    return arr


def auto_plan(lib, arr, count, chunk_capacity=64):
    """(items, chunks) of dxtlt_debug_plan_pixels_batch_auto at the cap in force on the thread"""
    items, chunks, n = (PlanItem * max(1, count))(), (PlanChunk * chunk_capacity)(), C.c_size_t(0)
    rc = lib.dxtlt_debug_plan_pixels_batch_auto(arr, count, items, chunks, chunk_capacity, C.byref(n))
    assert rc == 0 and n.value <= chunk_capacity, (rc, n.value, lib.dxtlt_last_error())
    return list(items[:count]), list(chunks[:n.value])
