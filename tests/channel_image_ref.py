"""Expected values of the BC4 / BC5 image decoders (docs/IMAGE_DECODE.md, "BC4 / BC5"), for the tests only.

Pixel i of a BC4 block B is the ALPHA byte of pixel i of the BC3 block whose first 8 bytes are B (docs/BC45_FORMAT.md section 1:
a BC4 block is byte for byte the alpha half of a BC3 block, a BC5 block two of them).  So every 8-byte half is padded to a BC3
block with 8 zero bytes, decoded with the oracle's BC3 decoder, and channel 3 taken."""
from __future__ import annotations

import functools

import numpy as np

BLOCK = {"bc4": 8, "bc5": 16}
BPP = {"bc4": 1, "bc5": 2}
FMT_ID = {"bc4": 4, "bc5": 5}


def blocks_of(width: int, height: int) -> int:
    return ((width + 3) // 4) * ((height + 3) // 4)


def decode_blocks(oracle, fmt: str, blocks) -> np.ndarray:
    """(n, 16, bpp): the sixteen pixels of every block, row-major, r (BC4) or r, g (BC5)"""
    halves = np.asarray(blocks, dtype=np.uint8).reshape(-1, 8)
    bc3 = np.zeros((halves.shape[0], 16), dtype=np.uint8)
    bc3[:, :8] = halves
    alpha = oracle.decode_blocks("bc3", bc3.reshape(-1)).reshape(-1, 16, 4)[:, :, 3]
    if fmt == "bc4":
        return np.ascontiguousarray(alpha.reshape(-1, 16, 1))
    return np.ascontiguousarray(alpha.reshape(-1, 2, 16).transpose(0, 2, 1))   # halves 2b, 2b + 1 = red, green of block b


def image_of(oracle, fmt: str, blocks, width: int, height: int) -> np.ndarray:
    """the expected height x width x bpp image of a block array in block order"""
    bx, by, bpp = (width + 3) // 4, (height + 3) // 4, BPP[fmt]
    px = decode_blocks(oracle, fmt, blocks).reshape(by, bx, 4, 4, bpp)   # block row, block column, pixel row, pixel column, channel
    return np.ascontiguousarray(px.transpose(0, 2, 1, 3, 4).reshape(4 * by, 4 * bx, bpp)[:height, :width])


def expected_buffer(image: np.ndarray, pitch: int) -> np.ndarray:
    """pitch * height bytes: the image's rows, 0xA5 everywhere else"""
    height, width, bpp = image.shape
    want = np.full((height, pitch), 0xA5, dtype=np.uint8)
    want[:, :bpp * width] = image.reshape(height, bpp * width)
    return want.reshape(-1)


@functools.lru_cache(maxsize=None)
def every_endpoint_pair() -> np.ndarray:
    """65 536 BC4 blocks, block p = (a0, a1) = (p >> 8, p & 255): its sixteen 3-bit indices are i mod 8 rotated by p, so every
    block uses all eight table entries.  Read as 32 768 BC5 blocks it pairs (a0, even a1) in red with (a0, a1 + 1) in green."""
    p = np.arange(65536, dtype=np.uint64)
    idx = (np.arange(16, dtype=np.uint64)[None, :] + p[:, None]) % 8
    bits = (idx << (3 * np.arange(16, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)   # 48 bits, pixel i at [3i, 3i + 2]
    word = (p >> 8) | ((p & 255) << 8) | (bits << 16)
    out = word.astype("<u8").view(np.uint8).copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def random_blocks(fmt: str, n: int, seed: int = 0) -> np.ndarray:
    """seeded random blocks: random endpoints are a0 <= a1 (the six-value table with 0 and 255) in half of the halves; every
    35th half has a0 == a1"""
    x = np.random.default_rng(0xC4A7 + 131 * n + FMT_ID[fmt] + 7919 * seed).integers(0, 256, n * BLOCK[fmt], dtype=np.uint8)
    halves = x.reshape(-1, 8)
    halves[::35, 1] = halves[::35, 0]
    x.setflags(write=False)
    return x
