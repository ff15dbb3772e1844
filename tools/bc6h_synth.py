#!/usr/bin/env python3
"""A small deterministic BC6H (UF16) encoder for measurements -- CPU only, no library, no GPU.

It is no quality encoder: per 4x4 block it takes the channel-wise min / max as endpoints, picks a two-region mode with the
best of the 32 partitions when that halves the block's channel spread, and otherwise a one-region mode; among the modes of
that kind it takes the one of highest endpoint precision whose stored deltas fit (docs/BC6H_FORMAT.md section 1 has the
field table, tests/bc6h_ref.py the packing).  That is enough to emit the mode mix a real encoder emits on smooth content:
one- and two-region blocks, transformed and untransformed modes.

    hdr_from_png(path)  -> H x W x 3 float32, an HDR image lifted from an 8-bit PNG (smooth, values up to ~40)
    encode(img)          -> N x 16 uint8 BC6H blocks (UF16), N = H W / 16, rows of blocks in raster order
    random_blocks(n, seed) -> n blocks of random bits with a random mode (the reserved encodings included)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bc6h_ref as R  # noqa: E402

ONE_REGION = (13, 12, 11, 10)                  # by base precision: 16, 12, 11, 10 bits
TWO_REGION = (2, 3, 4, 0, 5, 6, 7, 8, 1, 9)    # 11, 11, 11, 10, 9, 8, 8, 8, 7, 6 bits


def hdr_from_png(path: str, upscale: int = 2) -> np.ndarray:
    from PIL import Image

    im = Image.open(path).convert("RGB")
    if upscale > 1:
        im = im.resize((im.width * upscale, im.height * upscale), Image.BILINEAR)
    x = np.asarray(im).astype(np.float32) / 255.0
    h, w, _ = x.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    gain = 1.0 + 39.0 * np.exp(-(((xx - 0.3 * w) ** 2 + (yy - 0.35 * h) ** 2) / (0.08 * w * h)))   # a bright, smooth "sun"
    return (x ** 2.2) * gain[:, :, None]


def _quant(h: np.ndarray, bits: int) -> np.ndarray:
    """half bits (0..0x7BFF) -> a bits-bit endpoint whose unquantised value is closest below"""
    v = h.astype(np.int64) * 64 // 31
    if bits >= 16:
        return np.clip(v, 0, 0xFFFF)
    return np.clip((v << bits) >> 16, 0, (1 << bits) - 1)


def _indices(px: np.ndarray, lo: np.ndarray, hi: np.ndarray, ib: int) -> np.ndarray:
    """px (n, 16, 3), lo / hi (n, 16, 3) endpoints in half bits per pixel -> indices (n, 16)"""
    d = (hi - lo).astype(np.float64)
    t = ((px - lo) * d).sum(axis=2) / np.maximum((d * d).sum(axis=2), 1.0)
    return np.clip(np.rint(t * ((1 << ib) - 1)), 0, (1 << ib) - 1).astype(np.int64)


def encode(img: np.ndarray) -> np.ndarray:
    h, w, _ = img.shape
    half = np.clip(img, 0, 65504).astype(np.float16).view(np.uint16).astype(np.int64)
    px = half.reshape(h // 4, 4, w // 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 3)
    n = px.shape[0]
    masks = np.array(R.PARTITIONS, dtype=np.int64)
    sub = (masks[:, None] >> np.arange(16)[None, :]) & 1                                   # (32, 16)
    spread1 = (px.max(axis=1) - px.min(axis=1)).sum(axis=1)
    best_p, best_s = np.zeros(n, dtype=np.int64), np.full(n, np.iinfo(np.int64).max)
    for p in range(32):
        s = 0
        for r in (0, 1):
            m = sub[p].astype(bool) == bool(r)
            q = px[:, m]
            s = s + (q.max(axis=1) - q.min(axis=1)).sum(axis=1)
        better = s < best_s
        best_p[better], best_s[better] = p, s[better]
    two = best_s * 2 < spread1
    out = np.zeros((n, 16), dtype=np.uint8)
    for i in range(n):
        out[i] = _encode_block(px[i], two[i], int(best_p[i]), sub)
    return out


def _encode_block(p: np.ndarray, two: bool, part: int, sub: np.ndarray) -> np.ndarray:
    subsets = [sub[part] == 0, sub[part] == 1] if two else [np.ones(16, dtype=bool)]
    anchors = [0, R.ANCHOR2[part]] if two else [0]
    ib = 3 if two else 4
    for k in (TWO_REGION if two else ONE_REGION):
        epb = R.WIDTHS[k][0]
        ends, idx = [], np.zeros(16, dtype=np.int64)
        for r, m in enumerate(subsets):
            lo, hi = p[m].min(axis=0), p[m].max(axis=0)
            i = _indices(p[None, m], lo[None, None], hi[None, None], ib)[0]
            if i[np.nonzero(m)[0].tolist().index(anchors[r])] >> (ib - 1):   # the anchor's top index bit is not stored
                lo, hi, i = hi, lo, ((1 << ib) - 1) - i
            idx[m] = i
            ends += [_quant(lo, epb), _quant(hi, epb)]
        ep, fits = {}, True
        for ch in range(3):
            w0 = int(ends[0][ch])
            ep[(ch, 0)] = w0
            for e in range(1, len(ends)):
                v, dw = int(ends[e][ch]), R.field_width(k, ch, e)
                if R.TRANSFORMED[k]:
                    d = v - w0
                    if not -(1 << (dw - 1)) <= d < (1 << (dw - 1)):
                        fits = False
                    v = d & ((1 << dw) - 1)
                ep[(ch, e)] = v
        if fits or k in (9, 10):
            bits, at = 0, 0
            for px_i in range(16):
                nb = ib - 1 if px_i in anchors else ib
                bits |= int(idx[px_i]) << at
                at += nb
            return R.pack_block(k, ep, part if two else 0, bits)
    raise AssertionError("the untransformed modes always fit")


def random_blocks(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    k = rng.integers(0, 15, size=n)
    codes = np.array(R.MODE_BITS + (19,), dtype=np.uint8)
    mb = np.where(k <= 1, 3, 0x1F).astype(np.uint8)
    b[:, 0] = (b[:, 0] & ~mb) | codes[k]
    return b
