"""The method of tests/test_wide_offsets_gpu.py, written once: a pattern of P blocks tiled on the device to more than 2^28 lanes,
expected values from the CPU statements over the P pattern blocks only, byte-exact comparison on the device in chunks of at most
1 GiB, outputs inside 0xA5 guards that are counted on the device, every large array cut from one arena.  Nothing here copies more
than a few MiB to the host, and nothing depends on the device being a GPU: tests/test_wide_common.py runs the comparisons on CPU
tensors at small sizes."""
from __future__ import annotations

import numpy as np
import pytest
import torch

P = 4093                            # pattern blocks: prime, so coprime to 64, 256, 1024 and every blocks_per_row used
LANES = 2**28 + 3 * 256 + 77        # 2^20 + 4 workgroups of 256: a full first grid row, four workgroups in the second
FILL = 0xA5
GUARD = 4096                        # bytes of FILL in front of and behind every output
CHUNK = 1 << 30                     # bytes of output compared at a time, at most
GATHER = 1 << 25                    # rows gathered at a time, at most: torch launches one 64-lane workgroup per row of 16 bytes,
                                    # and 2^26 of them are 2^32 threads along x, which HIP refuses ("invalid configuration")
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16, "bc4": 8, "bc5": 16, "bc7": 16, "bc6h": 16}
BPP = {"bc1": 4, "bc2": 4, "bc3": 4, "bc4": 1, "bc5": 2, "bc7": 4, "bc6h": 8}
WIDE_BLOCKS_PER_ROW = 16411         # prime


ARENA = 53 << 30                    # the largest case: BC3 blocks and the twelve outputs of normalize_blocks_all_modes, 4 GiB each
SPARE = 8 << 30                     # what stays free beside the arena: the comparisons' temporaries and the library's own memory


class Arena:
    """One allocation that every large array of these tests is cut from.  A fresh allocation of tens of GiB costs the driver
    seconds (measured: 0.1 s per GiB, more than the kernels and the comparisons together), so the tests allocate once and `need`
    starts every case at the arena's front.  The arena is the card's free memory less SPARE, at most ARENA: a case that needs
    more skips -- the only skip of these tests -- which is the rule "less free memory than the case needs plus 8 GiB"."""

    def __init__(self, dev, nbytes=None):
        dev = torch.device(dev)
        self.free = None
        if nbytes is None:
            torch.cuda.empty_cache()   # memory cached from earlier tests counts as used in mem_get_info
            self.free, _ = torch.cuda.mem_get_info(dev)
            nbytes = max(0, min(ARENA, self.free - SPARE))
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 256 == 0 or not self.buf.is_cuda
        self.used = 0

    @property
    def device(self):
        return self.buf.device

    def need(self, nbytes, what):
        """start a case of `nbytes` (its large arrays; guards, alignment and small images are on top, under 4 MiB)"""
        self.used = 0
        if nbytes + (4 << 20) > self.buf.numel():
            pytest.skip(f"needs {nbytes / 2**30:.1f} GiB for {what} plus 8 GiB, {(self.free or 0) >> 30} GiB were free")

    def take(self, nbytes, off=0):
        """`nbytes` bytes at `off` bytes past the next 256-byte boundary (of the address: the arena starts on one)"""
        start = (self.used + 255) // 256 * 256 + off
        assert start + nbytes <= self.buf.numel(), "the case's `need` is too small"
        self.used = start + nbytes
        return self.buf[start:start + nbytes]


# ---- patterns ------------------------------------------------------------------------------------------------------------
def bcn_pattern(fmt, seed=0):
    """(P, block bytes) random BC1..BC5 blocks, about 1 in 8 "interesting": colour endpoints c0 <= c1 (BC1's punch-through mode;
    every 64th c0 == c1) and alpha endpoints a0 <= a1 (the six-value table); asserts that every class occurs"""
    bs = BLOCK[fmt]
    x = np.random.default_rng(0x51DE + 977 * seed + sum(map(ord, fmt))).integers(0, 256, (P, bs), dtype=np.uint8)
    if fmt in ("bc1", "bc2", "bc3"):
        at = 0 if fmt == "bc1" else 8
        c = x[:, at:at + 4].copy().view("<u2")
        lo, hi = c.min(axis=1), c.max(axis=1)
        c[:, 0], c[:, 1] = hi, lo                        # c0 >= c1 ...
        c[::8, 0], c[::8, 1] = lo[::8], hi[::8]           # ... but for every 8th
        c[::64, 1] = c[::64, 0]
        x[:, at:at + 4] = c.view(np.uint8)
        assert (c[:, 0] > c[:, 1]).any() and (c[:, 0] < c[:, 1]).any() and (c[:, 0] == c[:, 1]).any()
    if fmt in ("bc3", "bc4", "bc5"):
        for at in ((0,) if fmt != "bc5" else (0, 8)):
            a = x[:, at:at + 2].copy()
            lo, hi = a.min(axis=1), a.max(axis=1)
            x[:, at], x[:, at + 1] = hi, lo
            x[3::8, at], x[3::8, at + 1] = lo[3::8], hi[3::8]
            x[3::64, at + 1] = x[3::64, at]
            assert (x[:, at] > x[:, at + 1]).any() and (x[:, at] < x[:, at + 1]).any() and (x[:, at] == x[:, at + 1]).any()
    x.setflags(write=False)
    return x


def bc7_pattern(seed=7):
    import bc7_decode_ref as ref

    x = ref.mode_balanced_blocks(P, seed)
    assert set(ref.block_modes(x).tolist()) == set(range(8))
    x.setflags(write=False)
    return x


def bc6h_pattern(seed=6):
    import bc6h_decode_ref as ref

    x = ref.mode_balanced_blocks(P, seed)
    assert set(ref.block_classes(x).tolist()) == set(range(14))
    x.setflags(write=False)
    return x


def pattern_of(fmt):
    return bc7_pattern() if fmt == "bc7" else bc6h_pattern() if fmt == "bc6h" else bcn_pattern(fmt)


def decoded_pattern(oracle, fmt, pattern):
    """(P, 16 * bpp) bytes: the sixteen row-major pixels of every pattern block by the CPU statement of its format"""
    import bc6h_decode_ref
    import bc7_decode_ref
    import channel_image_ref

    flat = np.ascontiguousarray(pattern).reshape(-1)
    if fmt in ("bc1", "bc2", "bc3"):
        out = oracle.decode_blocks(fmt, flat)
    elif fmt in ("bc4", "bc5"):
        out = channel_image_ref.decode_blocks(oracle, fmt, flat)
    elif fmt == "bc7":
        out = bc7_decode_ref.decode_blocks(pattern)
    else:
        out = bc6h_decode_ref.records(bc6h_decode_ref.decode_blocks(pattern))
    out = np.ascontiguousarray(out, dtype=np.uint8).reshape(pattern.shape[0], 16 * BPP[fmt])
    rows = out.reshape(-1, 4 * BPP[fmt])
    assert not (rows == FILL).all(axis=1).any()   # no pixel row of a block looks like untouched output
    return out


# ---- device arrays -------------------------------------------------------------------------------------------------------
def tiled(pattern, n, arena, first=0, off=0, out=None):
    """n * rec bytes of the arena, `off` bytes past a 256-byte boundary (or the n * rec bytes `out`): element i is
    pattern[(first + i) % len(pattern)]"""
    period, rec = pattern.shape
    if out is None:
        out = arena.take(n * rec, off)
    assert out.numel() == n * rec
    pat = torch.from_numpy(np.ascontiguousarray(np.roll(pattern, -(first % period), axis=0))).to(out.device).reshape(-1)
    whole = n // period
    if whole:
        out[:whole * period * rec].view(whole, period * rec).copy_(pat.expand(whole, period * rec))
    out[whole * period * rec:].copy_(pat[:(n - whole * period) * rec])
    return out


class Guarded:
    """`n` bytes of the arena at `off` bytes past a 256-byte boundary, between GUARD + off bytes of 0xA5 in front and GUARD behind;
    0xA5 themselves, or a copy of `data`"""

    def __init__(self, arena, n, off=0, data=None):
        self.n, self.at = n, GUARD + off
        self.base = arena.take(self.at + n + GUARD)
        self.base.fill_(FILL)
        self.view = self.base[self.at:self.at + n]
        if data is not None:
            self.view.copy_(data)

    def check_guards(self):
        bad = int((self.base[:self.at] != FILL).sum()) + int((self.base[self.at + self.n:] != FILL).sum())
        assert bad == 0, f"{bad} guard bytes were written"


def count_not_fill(t):
    """bytes of the 1-D uint8 tensor that are not 0xA5, counted where the tensor lives"""
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    for lo in range(0, t.numel(), CHUNK):
        total += (t[lo:lo + CHUNK] != FILL).sum()
    return int(total)


def _report(got, want, first_element, rec, what):
    """got, want: (elements, rec) byte tensors that differ"""
    wrong = (got != want).reshape(got.shape[0], -1)
    e = int(torch.nonzero(wrong.any(dim=1))[0])
    byte = int(torch.nonzero(wrong[e])[0])
    pytest.fail(f"{what}: first wrong element {first_element + e}, byte {byte} of it, byte offset {(first_element + e) * rec + byte}: "
                f"got {got[e].reshape(-1)[:16].tolist()}.., want {want[e].reshape(-1)[:16].tolist()}..")


def check_records(out, expected, n, what, first=0, chunk=CHUNK):
    """`out`: n * rec bytes, record i must be expected[(first + i) % len(expected)]; `expected` a (P, rec) tensor on out's device"""
    rec, period = expected.shape[1], expected.shape[0]
    assert out.numel() == n * rec
    got = out.view(n, rec)
    step = max(1, min(chunk // rec, GATHER))
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        want = expected[(torch.arange(lo, hi, device=out.device) + first) % period]
        if not torch.equal(got[lo:hi], want):
            _report(got[lo:hi], want, lo, rec, what)


def check_image(out, pitch, width, height, bpp, expected, what, first=0, chunk=CHUNK):
    """`out`: pitch * (height - 1) + bpp * width bytes or more, a row-major image whose block b (row-major over ceil(width / 4)
    columns) must be expected[(first + b) % len(expected)] cut to the image; every byte between the rows must still be 0xA5.
    The width is a multiple of 4 (the tests that need a clipped column use small images, checked on the host)."""
    assert width % 4 == 0
    bpr, row_bytes, period = width // 4, bpp * width, expected.shape[0]
    assert expected.shape[1] == 16 * bpp and pitch >= row_bytes
    per_chunk = max(1, min(chunk // (4 * pitch), GATHER // bpr))
    block_rows = (height + 3) // 4
    for r0 in range(0, block_rows, per_chunk):
        r1 = min(block_rows, r0 + per_chunk)
        rows = min(height, 4 * r1) - 4 * r0                       # pixel rows of the chunk; the image's last block row may be clipped
        want = expected[(torch.arange(r0 * bpr, r1 * bpr, device=out.device) + first) % period].view(r1 - r0, bpr, 4, 4 * bpp)
        want_rows = want.permute(0, 2, 1, 3).reshape(4 * (r1 - r0), row_bytes)[:rows]   # pixel row, then block column
        at = 4 * r0 * pitch
        whole = rows if r1 < block_rows else rows - 1             # rows with their `pitch` bytes: all but the image's last
        assert out.numel() >= at + whole * pitch + (row_bytes if whole < rows else 0)
        if whole:
            body = out[at:at + whole * pitch].view(whole, pitch)
            gap = int((body[:, row_bytes:] != FILL).sum())
            assert gap == 0, f"{what}: {gap} bytes between the rows of block rows [{r0}, {r1}) were written"
            if not torch.equal(body[:, :row_bytes], want_rows[:whole]):
                _image_report(body[:, :row_bytes], want_rows[:whole], 4 * r0, pitch, bpp, what)
        if whole < rows:
            last = out[at + whole * pitch:at + whole * pitch + row_bytes].view(1, row_bytes)
            if not torch.equal(last, want_rows[whole:]):
                _image_report(last, want_rows[whole:], 4 * r0 + whole, pitch, bpp, what)


def _image_report(got, want, first_row, pitch, bpp, what):
    wrong = got != want
    y = int(torch.nonzero(wrong.any(dim=1))[0])
    xb = int(torch.nonzero(wrong[y])[0])
    pytest.fail(f"{what}: first wrong pixel ({xb // bpp}, {first_row + y}), byte offset {(first_row + y) * pitch + xb}: "
                f"got {got[y, xb:xb + 16].tolist()}, want {want[y, xb:xb + 16].tolist()}")


def small_image_bytes(decoded, width, height, bpp):
    """(height, bpp * width) numpy bytes of the image whose blocks are the (n, 16 * bpp) `decoded`, clipped"""
    bw, bh = (width + 3) // 4, (height + 3) // 4
    px = np.asarray(decoded, dtype=np.uint8)[:bw * bh].reshape(bh, bw, 4, 4 * bpp)
    return np.ascontiguousarray(px.transpose(0, 2, 1, 3).reshape(4 * bh, 4 * bw * bpp)[:height, :bpp * width])


def check_small_image(g: Guarded, pitch, width, height, bpp, want_rows, what):
    """the image at the start of the Guarded payload against `want_rows` (height, bpp * width) on the host, then -- its rows
    put back to 0xA5 -- not one byte of the whole allocation may differ from 0xA5.  Spoils the output."""
    row_bytes = bpp * width
    starts = torch.arange(height, device=g.base.device, dtype=torch.int64) * pitch + g.at
    index = (starts[:, None] + torch.arange(row_bytes, device=g.base.device, dtype=torch.int64)[None, :]).reshape(-1)
    got = g.base[index].cpu().numpy().reshape(height, row_bytes)
    if not np.array_equal(got, want_rows):
        y, x = np.argwhere(got != want_rows)[0]
        pytest.fail(f"{what}: first wrong pixel ({x // bpp}, {y}), byte offset {int(y) * pitch + int(x)}: got {got[y, x:x + 16].tolist()}, "
                    f"want {want_rows[y, x:x + 16].tolist()}")
    g.base[index] = FILL
    stray = count_not_fill(g.base)
    assert stray == 0, f"{what}: {stray} bytes outside the image's rows were written"
