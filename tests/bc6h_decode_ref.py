"""The numpy statement of the BC6H (UF16) decoder to RGBA16F pixels (docs/IMAGE_DECODE.md, "BC6H blocks to a row-major RGBA16F
image"), for the tests and tools.  The values are those of tests/bc6h_ref.py `decode(blocks, signed=False)`, which
tests/test_bc6h.py pins to Pillow mode by mode; this module adds the alpha half, the 128-byte record of a block, the row-major
image with its clipping, Pillow's half -> 8-bit map, the block generators of the decode tests and -- `decode_field_table()` --
the generated part of csrc/bc6h_decode_fields.h.  Signed (SF16) decoding is not stated here (the document has the reason)."""
from __future__ import annotations

import numpy as np

import bc6h_ref

ONE = 0x3C00            # 1.0 as a half: every pixel's alpha
CLASSES = bc6h_ref.CLASSES
RESERVED = bc6h_ref.RESERVED
RESERVED_MODE_BITS = (19, 23, 27, 31)


def decode_blocks(blocks) -> np.ndarray:
    """(n, 16) blocks -> (n, 16 pixels, 4) half-float bit patterns r, g, b, a (uint16); pixel 4 r + c is (c, r)"""
    blocks = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint8).reshape(-1, 16))
    out = np.empty((blocks.shape[0], 16, 4), dtype=np.uint16)
    out[:, :, :3] = bc6h_ref.decode(blocks, signed=False)
    out[:, :, 3] = ONE
    return out


def records(pixels) -> np.ndarray:
    """(n, 16, 4) halves -> the (n, 128) bytes of the block-array call: sixteen pixels of four little-endian halves"""
    return np.ascontiguousarray(np.asarray(pixels, dtype=np.uint16).astype("<u2")).view(np.uint8).reshape(-1, 128)


def image_of(pixels, width: int, height: int) -> np.ndarray:
    """(height, width, 4) uint16 image of the row-major blocks' (n, 16, 4) pixels; blocks beyond the edge are clipped"""
    bw, bh = (width + 3) // 4, (height + 3) // 4
    px = np.asarray(pixels, dtype=np.uint16)[:bw * bh].reshape(bh, bw, 4, 4, 4)
    return np.ascontiguousarray(px.transpose(0, 2, 1, 3, 4).reshape(4 * bh, 4 * bw, 4)[:height, :width])


def image_bytes(pixels, width: int, height: int) -> np.ndarray:
    """the image as (height, 8 * width) bytes: pixel (x, y) at row y, byte 8 x"""
    return image_of(pixels, width, height).astype("<u2").view(np.uint8).reshape(height, 8 * width)


def pillow_8bit(halves) -> np.ndarray:
    """Pillow's own map of a decoded BC6H channel to 8 bits: half -> float32, below 0 -> 0, above 1 -> 255, else trunc(255 v)"""
    v = np.asarray(halves, dtype=np.uint16).view(np.float16).astype(np.float32)
    return np.where(v < 0, 0, np.where(v > 1, 255, np.trunc(np.float32(255) * np.clip(v, 0, 1)))).astype(np.uint8)


# ---- block generators --------------------------------------------------------------------------------------------------
def block_classes(blocks) -> np.ndarray:
    return bc6h_ref.block_class(np.asarray(blocks, dtype=np.uint8).reshape(-1, 16)[:, 0])


def with_class(blocks, classes) -> np.ndarray:
    """the (n, 16) blocks with the mode bits of `classes` (0..13; 14 = one of the four reserved values, picked by the bits
    that were there) in byte 0, the other bits as they are"""
    blocks = np.array(blocks, dtype=np.uint8).reshape(-1, 16)
    classes = np.asarray(classes, dtype=np.int64)
    mode = np.array(bc6h_ref.MODE_BITS + (0,), dtype=np.int64)[classes]
    mode = np.where(classes == RESERVED, 19 + 4 * ((blocks[:, 0].astype(np.int64) >> 2) & 3), mode)
    keep = np.where(classes <= 1, 0xFC, 0xE0)
    blocks[:, 0] = (blocks[:, 0] & keep) | mode
    assert np.array_equal(block_classes(blocks), classes)
    return blocks


def _random(n, seed):
    rng = np.random.default_rng(seed)
    return rng, rng.integers(0, 256, (n, 16), dtype=np.uint8)


def mode_balanced_blocks(n, seed):
    """random blocks whose class is drawn uniformly from the 14 modes (plain random bytes are half classes 0 and 1)"""
    rng, blocks = _random(n, seed)
    return with_class(blocks, rng.integers(0, 14, n))


def single_class_blocks(n, cls, seed):
    return with_class(_random(n, seed)[1], np.full(n, cls))


def wave_uniform_blocks(n, seed):
    """every run of 64 blocks of one class, each of the fifteen classes in turn"""
    return with_class(_random(n, seed)[1], (np.arange(n) // 64) % CLASSES)


def interleaved_class_blocks(n, seed):
    """all fifteen classes, the reserved values included, side by side in every wave"""
    return with_class(_random(n, seed)[1], np.arange(n) % CLASSES)


def reserved_blocks(n, seed):
    blocks = with_class(_random(n, seed)[1], np.full(n, RESERVED))
    assert set((blocks[:, 0] & 0x1F).tolist()) == set(RESERVED_MODE_BITS)
    return blocks


# ---- the decoder's field table (csrc/bc6h_decode_fields.h) ----------------------------------------------------------------
def field_runs(k: int):
    """the endpoint fields of class k as (channel, endpoint, block bit, value bit, length) runs of consecutive bits, in the
    order red w x y z, green ..., blue ..."""
    out = []
    for ch in range(3):
        for e in range(bc6h_ref.n_endpoints(k)):
            pos = bc6h_ref.FIELDS[k][(ch, e)]
            i = 0
            while i < len(pos):
                j = i + 1
                while j < len(pos) and pos[j] == pos[j - 1] + 1:
                    j += 1
                out.append((ch, e, pos[i], i, j - i))
                i = j
    return out


def decode_field_table() -> str:
    """the generated part of csrc/bc6h_decode_fields.h"""
    lines = []
    for k in range(14):
        bits, dr, dg, db = bc6h_ref.WIDTHS[k]
        runs = ", ".join("{%d, %d, %d, %d, %d}" % r for r in field_runs(k))
        lines.append(f"template <> struct DecodeTab<{k}> {{")
        lines.append(f"    static constexpr int bits = {bits}, delta[3] = {{{dr}, {dg}, {db}}};")
        lines.append(f"    static constexpr bool transformed = {str(bc6h_ref.TRANSFORMED[k]).lower()}, "
                     f"two_regions = {str(bc6h_ref.two_region(k)).lower()};")
        lines.append(f"    static constexpr FieldRun runs[] = {{{runs}}};")
        lines.append("};")
    return "\n".join(lines) + "\n"
