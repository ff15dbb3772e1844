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
