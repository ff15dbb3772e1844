"""The data sets the pixel auto transform's choice is held to (docs/PIXEL_FORMAT.md "The auto transform"), each as an (P, B) uint8
array with the 1-based index of the candidate that zlib-6 compresses smallest, in the order of entropy_ref.CANDIDATES.  Built once
per process; the tests never write into them."""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@functools.lru_cache(maxsize=None)
def r2_256_rgba() -> np.ndarray:
    """the 256 x 256 RGBA image the golden BC7 payload decodes to"""
    import bc7_decode_ref

    blocks = np.fromfile(os.path.join(ROOT, "tests", "golden", "r2-256-bc7.payload.bin"), dtype=np.uint8)
    img = bc7_decode_ref.image_of(bc7_decode_ref.decode_blocks(blocks), 256, 256)
    img.setflags(write=False)
    return img


def random_walks(channels: int, pixels: int = 65536, seed: int = 0x3A1C) -> np.ndarray:
    """`channels` independent random walks: steps in -2..2, clipped to +-120 around 128"""
    rng = np.random.default_rng(seed)
    out = np.empty((pixels, channels), dtype=np.uint8)
    for c in range(channels):
        steps = rng.integers(-2, 3, pixels)
        v, walk = 0, np.empty(pixels, dtype=np.int64)
        for i, s in enumerate(steps.tolist()):
            v = max(-120, min(120, v + s))
            walk[i] = v
        out[:, c] = 128 + walk
    return out


@functools.lru_cache(maxsize=None)
def data_sets():
    """[(name, (P, B) pixels, expected 1-based pick)]"""
    from tools import pixels_gain

    img = r2_256_rgba()
    syn = pixels_gain.synthetic(512, 0x9155).reshape(-1, 4)
    sets = [
        ("r2-256 RGBA", img.reshape(-1, 4), 1),
        ("r2-256 RGB", img.reshape(-1, 4)[:, :3], 1),
        ("r2-256 mip chain", pixels_gain.mip_chain(img), 1),
        ("synthetic RGBA", syn, 4),
        ("synthetic RGB", syn[:, :3], 4),
        ("random walks x4", random_walks(4), 4),
        ("random walks x3", random_walks(3), 4),
    ]
    out = []
    for name, px, want in sets:
        px = np.ascontiguousarray(px)
        px.setflags(write=False)
        out.append((name, px, want))
    return out


WINNER_PIXELS = 16384      # two windows interleaved for B = 4; a plane is half a window


@functools.lru_cache(maxsize=None)
def winner_sets():
    """[(name, B, (16384, B) pixels, index of the candidate that wins STRICTLY under entropy_ref.auto)]: one input per candidate
    and pixel size, B = 4 first.  Candidates 0 and 3 are the head of the r2-256 mip chain and random walks; the other four are
    drawn from ONE default_rng(5), in this order (the seed and the order are part of the construction):
      5 (plain, INTERLEAVED)        every channel uniform over 16 values, one set of 16 in the first half of the pixels and a disjoint
                                    set in the second: interleaved windows see one set each, a plane sees both
      1 (decorrelate, PLANAR)       green uniform bytes, red and blue green + 0..3, alpha 0..3: subtract-green leaves two bits, and
                                    planes keep them away from green
      2 (decorrelate, INTERLEAVED)  green from the two half-sets, red and blue green + one of four values of the half's own set,
                                    alpha = green
      4 (plain, PLANAR)             channel c uniform over eight multiples of c + 3: every plane has its own eight values"""
    P, h = WINNER_PIXELS, WINNER_PIXELS // 2
    rng = np.random.default_rng(5)
    sets = (np.arange(16, dtype=np.uint8) * 3 + 10, np.arange(16, dtype=np.uint8) * 5 + 120)
    assert not set(sets[0].tolist()) & set(sets[1].tolist())

    def halves(channels, pools):
        px = np.empty((P, channels), np.uint8)
        px[:h] = rng.choice(pools[0], (h, channels))
        px[h:] = rng.choice(pools[1], (P - h, channels))
        return px

    chain = np.ascontiguousarray(data_sets()[2][1])
    out = []
    for B in (4, 3):
        interleaved = halves(B, sets)
        green = rng.integers(0, 256, P).astype(np.uint8)
        planar = np.empty((P, B), np.uint8)
        planar[:, 1] = green
        planar[:, 0] = green + rng.integers(0, 4, P).astype(np.uint8)
        planar[:, 2] = green + rng.integers(0, 4, P).astype(np.uint8)
        if B == 4:
            planar[:, 3] = rng.integers(0, 4, P).astype(np.uint8)
        green = halves(1, sets)[:, 0]
        small = (sets[0][:4], sets[1][:4])
        dec_interleaved = np.empty((P, B), np.uint8)
        dec_interleaved[:, 1] = green
        for c in (0, 2):
            dec_interleaved[:, c] = green + np.concatenate([rng.choice(small[0], h), rng.choice(small[1], P - h)]).astype(np.uint8)
        if B == 4:
            dec_interleaved[:, 3] = green
        plain_planar = np.stack([rng.choice(np.arange(8, dtype=np.uint8) * (c + 3), P) for c in range(B)], axis=1)
        for name, px, want in ((f"mip chain {B}", chain[:P, :B], 0), (f"green + 0..3 {B}", planar, 1), (f"half sets + green {B}", dec_interleaved, 2),
                               (f"random walks {B}", random_walks(B, P, 11 + B), 3), (f"multiples {B}", plain_planar, 4),
                               (f"half sets {B}", interleaved, 5)):
            px = np.ascontiguousarray(px)
            px.setflags(write=False)
            out.append((name, B, px, want))
    return out


@functools.lru_cache(maxsize=None)
def small_sets():
    """the same sets at 128 x 128 (crops of the images, the mip chain of the crop, the first 16384 pixels of the walks)"""
    from tools import pixels_gain

    crop = np.ascontiguousarray(r2_256_rgba()[64:192, 64:192])
    syn = np.ascontiguousarray(pixels_gain.synthetic(512, 0x9155)[192:320, 192:320]).reshape(-1, 4)
    sets = [
        ("r2-256 crop RGBA", crop.reshape(-1, 4)),
        ("r2-256 crop RGB", crop.reshape(-1, 4)[:, :3]),
        ("r2-256 crop mip chain", pixels_gain.mip_chain(crop)),
        ("synthetic crop RGBA", syn),
        ("synthetic crop RGB", syn[:, :3]),
        ("random walks x4", random_walks(4)[:16384]),
        ("random walks x3", random_walks(3)[:16384]),
    ]
    return [(name, np.ascontiguousarray(px)) for name, px in sets]
