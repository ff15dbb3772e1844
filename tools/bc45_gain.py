#!/usr/bin/env python3
"""What the BC4 / BC5 layout (docs/BC45_FORMAT.md) does to compressed size -- CPU only, no library, no GPU.

Data: BC4 / BC5 blocks made by a small deterministic min/max encoder (below) from
  * the luminance of r2-256.png, the image the reference's BC1-3 / BC7 test textures were made from (BC4),
  * X / Y of a tangent-space normal map derived from that luminance as a height field (BC5, and its X channel as BC4),
  * a seeded synthetic normal map, 1024 x 1024, from a smooth random height field (BC5, and its X channel as BC4).
For every data set and setting it prints the zlib-6 and zstd-1 (system libzstd through ctypes, tools/zstd_ratio.py) size of the
plain blocks and of the transformed ones, and the gain (1 - transformed / plain), as ONE JSON line.
    python tools/bc45_gain.py [path/to/r2-256.png]
The image is read from the path given (default: the reference tree's tests/assets); without it only the synthetic set runs."""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bc45_ref  # noqa: E402
from tools import zstd_ratio  # noqa: E402

DEFAULT_PNG = "/root/reference/src/assets/tests/r2-256.png"


def encode_bc4(channel: np.ndarray) -> np.ndarray:
    """min/max BC4: a0 = block max, a1 = block min (a0 > a1: the eight-value palette), every texel to its nearest palette entry;
    a flat block is a0 = a1 with all indices 0.  channel: H x W uint8, H and W multiples of 4."""
    h, w = channel.shape
    t = channel.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16).astype(np.int32)
    a0, a1 = t.max(axis=1), t.min(axis=1)
    # palette of the a0 > a1 mode: a0, a1, then (6 - i) / 7 a0 + (i + 1) / 7 a1 -- rounded as decoders do
    k = np.arange(6)
    inner = ((6 - k)[None, :] * a0[:, None] + (k + 1)[None, :] * a1[:, None] + 3) // 7
    pal = np.concatenate([a0[:, None], a1[:, None], inner], axis=1)                # n x 8
    idx = np.abs(t[:, :, None] - pal[:, None, :]).argmin(axis=2).astype(np.uint64)  # n x 16, first nearest wins
    idx[a0 == a1] = 0
    bits = np.zeros(len(t), dtype=np.uint64)
    for i in range(16):
        bits |= idx[:, i] << np.uint64(3 * i)
    out = np.zeros((len(t), 8), dtype=np.uint8)
    out[:, 0], out[:, 1] = a0, a1
    for b in range(6):
        out[:, 2 + b] = ((bits >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    return out.reshape(-1)


def encode_bc5(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    return np.concatenate([encode_bc4(x).reshape(-1, 8), encode_bc4(y).reshape(-1, 8)], axis=1).reshape(-1)


def normal_map(height: np.ndarray, strength: float):
    """X, Y of the unit normal of a height field (central differences, wrap-around), as unsigned bytes"""
    hgt = height.astype(np.float64)
    dx = (np.roll(hgt, -1, axis=1) - np.roll(hgt, 1, axis=1)) * strength
    dy = (np.roll(hgt, -1, axis=0) - np.roll(hgt, 1, axis=0)) * strength
    nz = 1.0 / np.sqrt(dx * dx + dy * dy + 1.0)
    to8 = lambda v: np.clip(np.rint((v * nz * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)
    return to8(-dx), to8(-dy)


def synthetic_height(size: int, seed: int) -> np.ndarray:
    """a smooth random height field: a sum of 24 seeded sinusoids with falling amplitudes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
    h = np.zeros((size, size))
    for i in range(24):
        fx, fy = rng.integers(1, 3 + i, 2)
        h += np.sin(2 * np.pi * (fx * xx + fy * yy) + rng.uniform(0, 2 * np.pi)) / (1 + i)
    return (h - h.min()) / (h.max() - h.min()) * 255.0


def sizes(buf: bytes):
    return {"zlib6": len(zlib.compress(buf, 6)), "zstd1": zstd_ratio.compressed_size(buf, 1) if zstd_ratio.available() else None}


def measure(name: str, fmt: str, blocks: np.ndarray):
    plain = sizes(blocks.tobytes())
    row = {"data": name, "format": fmt, "bytes": int(blocks.size), "plain": plain, "settings": []}
    for split in (False, True):
        t = bc45_ref.transform(fmt, blocks, split)
        assert np.array_equal(bc45_ref.untransform(fmt, t, split), blocks)
        s = sizes(t.tobytes())
        row["settings"].append({"split_endpoints": split, **{k: v for k, v in s.items()},
                                **{f"gain_{k}_pct": (round(100.0 * (1 - s[k] / plain[k]), 2) if s[k] else None) for k in s}})
    return row


def main():
    png = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_PNG
    rows = []
    if os.path.exists(png):
        from PIL import Image

        rgb = np.asarray(Image.open(png).convert("RGB")).astype(np.float64)
        lum = np.clip(np.rint(0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]), 0, 255).astype(np.uint8)
        nx, ny = normal_map(lum, 2.0 / 255.0 * 4.0)
        rows.append(measure("r2-256 luminance", "bc4", encode_bc4(lum)))
        rows.append(measure("r2-256 normal X", "bc4", encode_bc4(nx)))
        rows.append(measure("r2-256 normal XY", "bc5", encode_bc5(nx, ny)))
    sx, sy = normal_map(synthetic_height(1024, 0xBC45), 1.0 / 4.0)
    rows.append(measure("synthetic normal X (seed 0xBC45, 1024^2)", "bc4", encode_bc4(sx)))
    rows.append(measure("synthetic normal XY (seed 0xBC45, 1024^2)", "bc5", encode_bc5(sx, sy)))
    print(json.dumps({"tool": "bc45_gain", "zstd_version": zstd_ratio.version() if hasattr(zstd_ratio, "version") else None,
                      "image": png if os.path.exists(png) else None, "rows": rows}))


if __name__ == "__main__":
    main()
