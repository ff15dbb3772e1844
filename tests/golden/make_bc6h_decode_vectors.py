"""Writes tests/golden/bc6h_decode_vectors.npz: BC6H (UF16) blocks and what Pillow's decoder (an implementation independent of
this project) makes of them.  Run once, by hand, where Pillow is installed; no test runs it.

    python tests/golden/make_bc6h_decode_vectors.py

blocks (N x 16 u8), pixels (N x 16 x 3 u8: Pillow's 8-bit r, g, b of pixel 4 r + c at (c, r), from a DX10 DDS file of DXGI format
95, BC6H_UF16).  Per mode: every partition of a two-region mode with one random and two low fills; all-zero and all-ones endpoint
fields; all-zero and all-ones index bits over random and over low endpoints, so that both endpoints of every subset reach a
pixel unmixed; random fills; and low fills.  A LOW fill has base endpoints whose top bit is clear and whose next bit is set,
and deltas small enough to keep every endpoint there, so that the decoded values lie between 1 / 255 and 1.0 or just above:
Pillow's 8-bit answer is 0 below the first and 255 from the second on, and a saturated channel pins nothing beyond the sign of an
error (a half float's bit patterns are logarithmic: the lower 45 % of the patterns below 1.0 are all below 1 / 255).  No block is
of the reserved mode values."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bc6h_ref as R  # noqa: E402

RANDOM_FILLS, LOW_FILLS = 24, 64


def pillow_rgb8(blocks):
    """(N, 16, 3) uint8: Pillow's decoding of the (N, 16) blocks, laid side by side in one 4-pixel-high image"""
    n = blocks.shape[0]
    image = Image.open(io.BytesIO(R.dds_dx10(blocks.tobytes(), 4 * n, 4, dxgi=95))).convert("RGB")
    return np.asarray(image, dtype=np.uint8).reshape(4, n, 4, 3).transpose(1, 0, 2, 3).reshape(n, 16, 3).copy()


def random_fields(rng, k):
    return {(ch, e): int(rng.integers(0, 1 << R.field_width(k, ch, e))) for ch in range(3) for e in range(R.n_endpoints(k))}


def low_fields(rng, k):
    """every endpoint in [2^(bits - 2), 2^(bits - 1)): the base endpoints drawn there, the deltas small enough to stay there"""
    bits = R.WIDTHS[k][0]
    top = 1 << (bits - 1)
    ep = {}
    for ch in range(3):
        dw = R.field_width(k, ch, 1)
        if not R.TRANSFORMED[k]:
            for e in range(R.n_endpoints(k)):
                ep[(ch, e)] = int(rng.integers(top // 2, top))
            continue
        reach = min(1 << (dw - 2), top // 8)            # |delta| <= reach - 1
        ep[(ch, 0)] = int(rng.integers(top // 2 + reach, top - reach))
        for e in range(1, R.n_endpoints(k)):
            ep[(ch, e)] = int(rng.integers(-(reach - 1), reach)) & ((1 << dw) - 1)
    return ep


def index_bits(rng):
    return int.from_bytes(rng.integers(0, 256, 8, dtype=np.uint8).tobytes(), "little")


def main():
    rng = np.random.default_rng(0xBC6D)
    blocks = []
    for k in range(14):
        partitions = range(32) if R.two_region(k) else [0]
        part = lambda: int(rng.integers(0, 32))                     # noqa: E731
        for p in partitions:
            blocks.append(R.pack_block(k, random_fields(rng, k), p, index_bits(rng)))
            blocks.append(R.pack_block(k, low_fields(rng, k), p, index_bits(rng)))
            blocks.append(R.pack_block(k, low_fields(rng, k), p, index_bits(rng)))
        for fill in (0, -1):
            for _ in range(2):
                ep = {key: fill & ((1 << R.field_width(k, *key)) - 1) for key in random_fields(rng, k)}
                blocks.append(R.pack_block(k, ep, part(), index_bits(rng)))
        for bits in (0, (1 << 64) - 1):
            for _ in range(2):
                blocks.append(R.pack_block(k, random_fields(rng, k), part(), bits))
                blocks.append(R.pack_block(k, low_fields(rng, k), part(), bits))
        for _ in range(RANDOM_FILLS):
            blocks.append(R.pack_block(k, random_fields(rng, k), part(), index_bits(rng)))
        for _ in range(LOW_FILLS):
            blocks.append(R.pack_block(k, low_fields(rng, k), part(), index_bits(rng)))
    blocks = np.stack(blocks)
    assert (R.block_class(blocks[:, 0]) < 14).all()
    pixels = pillow_rgb8(blocks)
    inside = ((pixels > 0) & (pixels < 255)).mean()
    np.savez_compressed(os.path.join(HERE, "bc6h_decode_vectors.npz"), blocks=blocks, pixels=pixels)
    print(blocks.shape[0], "blocks;", "%.3f" % inside, "of the channels strictly between 0 and 255")


if __name__ == "__main__":
    main()
