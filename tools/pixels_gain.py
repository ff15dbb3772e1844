#!/usr/bin/env python3
"""What the pixel layouts (docs/PIXEL_FORMAT.md) do to compressed size -- CPU only, no library, no GPU.

Data, each as RGBA8888 and as RGB888 (BGR order makes no difference to the transform: byte 1 is G either way):
  * r2-256.png, the image the reference's test textures were made from: its 256 x 256 top level, and the top level followed by
    its box-filtered mip chain down to 1 x 1 (87 381 pixels, an odd count);
  * a seeded synthetic texture, 512 x 512: smooth colour fields with correlated channels, grain, and a two-level alpha mask.
For every data set it prints the zlib-6 and zstd-3 (system libzstd through ctypes, tools/zstd_ratio.py) size of the plain pixels
and of all six settings, and the change against plain in percent (negative = smaller), as ONE JSON line.
    python tools/pixels_gain.py [path/to/r2-256.png] > profiles/pixels_gain.json
The image is read from the path given (default: where tools/bc45_gain.py looks); without it only the synthetic set runs."""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pixels_ref  # noqa: E402
from tools import zstd_ratio  # noqa: E402
from tools.bc45_gain import DEFAULT_PNG  # noqa: E402

LAYOUT_NAMES = ("INTERLEAVED", "PLANAR", "PLANAR_DELTA")


def mip_chain(rgba: np.ndarray) -> np.ndarray:
    """the level and every 2 x 2 box-filtered level below it down to 1 x 1 (rounded to nearest), pixels concatenated"""
    levels, cur = [rgba.reshape(-1, rgba.shape[2])], rgba.astype(np.uint32)
    while cur.shape[0] > 1 or cur.shape[1] > 1:
        h, w = max(1, cur.shape[0] // 2), max(1, cur.shape[1] // 2)
        ys, xs = (2 if cur.shape[0] > 1 else 1), (2 if cur.shape[1] > 1 else 1)
        cur = (cur[:h * ys, :w * xs].reshape(h, ys, w, xs, -1).sum(axis=(1, 3)) + (ys * xs) // 2) // (ys * xs)
        levels.append(cur.astype(np.uint8).reshape(-1, cur.shape[2]))
    return np.concatenate(levels)


def synthetic(size: int, seed: int) -> np.ndarray:
    """size x size RGBA: a smooth luminance field shared by the channels, a small smooth tint per channel, +-2 of grain, alpha
    255 inside a disc and 0 outside"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size

    def field(terms, amplitude):
        f = np.zeros((size, size))
        for i in range(terms):
            fx, fy = rng.integers(1, 3 + i, 2)
            f += np.sin(2 * np.pi * (fx * xx + fy * yy) + rng.uniform(0, 2 * np.pi)) / (1 + i)
        return f / np.abs(f).max() * amplitude

    lum = 128 + field(20, 100)
    out = np.zeros((size, size, 4), dtype=np.uint8)
    for c in range(3):
        out[..., c] = np.clip(np.rint(lum + field(6, 20) + rng.integers(-2, 3, (size, size))), 0, 255)
    out[..., 3] = np.where((xx - 0.5) ** 2 + (yy - 0.5) ** 2 < 0.2, 255, 0)
    return out


def sizes(buf: bytes):
    return {"zlib6": len(zlib.compress(buf, 6)), "zstd3": zstd_ratio.compressed_size(buf, 3) if zstd_ratio.available() else None}


def measure(name: str, px: np.ndarray):
    """px: P x B uint8"""
    B = px.shape[1]
    flat = np.ascontiguousarray(px).reshape(-1)
    plain = sizes(flat.tobytes())
    row = {"data": name, "pixel_bytes": B, "pixels": int(px.shape[0]), "plain": plain, "settings": []}
    for decorrelate, layout in pixels_ref.SETTINGS:
        t = pixels_ref.forward(flat, B, decorrelate, layout)
        assert np.array_equal(pixels_ref.inverse(t, B, decorrelate, layout), flat)
        s = sizes(t.tobytes())
        row["settings"].append({"decorrelate": decorrelate, "layout": LAYOUT_NAMES[layout], **s,
                                **{f"change_{k}_pct": (round(100.0 * (s[k] / plain[k] - 1), 2) if s[k] else None) for k in s}})
    return row


def main():
    png = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_PNG
    rows = []
    if os.path.exists(png):
        from PIL import Image

        rgba = np.asarray(Image.open(png).convert("RGBA"))
        chain = mip_chain(rgba)
        rows.append(measure("r2-256 top level, RGBA", rgba.reshape(-1, 4)))
        rows.append(measure("r2-256 top level, RGB", rgba.reshape(-1, 4)[:, :3]))
        rows.append(measure("r2-256 mip chain, RGBA", chain))
        rows.append(measure("r2-256 mip chain, RGB", chain[:, :3]))
    syn = synthetic(512, 0x9155)
    rows.append(measure("synthetic (seed 0x9155, 512^2), RGBA", syn.reshape(-1, 4)))
    rows.append(measure("synthetic (seed 0x9155, 512^2), RGB", syn.reshape(-1, 4)[:, :3]))
    print(json.dumps({"tool": "pixels_gain", "zstd_version": zstd_ratio.version(), "image": os.path.basename(png) if os.path.exists(png) else None,
                      "rows": rows}))


if __name__ == "__main__":
    main()
