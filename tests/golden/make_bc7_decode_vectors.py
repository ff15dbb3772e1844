"""Writes tests/golden/bc7_decode_vectors.npz and tests/golden/bc7_decode_digests.json: BC7 blocks and what Pillow's decoder
(an implementation independent of this project) makes of them.  Run once, by hand, where Pillow is installed; no test runs it.

    python tests/golden/make_bc7_decode_vectors.py

blocks (N x 16 u8), pixels (N x 64 u8: sixteen r, g, b, a pixels, pixel 4 r + c at (c, r)).  Per mode: every partition value the
mode has, every rotation x index selector; per such combination one block with all-zero and one with all-one endpoint fields
and four seeded random fills of the remaining bits.  No block is of the reserved encoding, for which Pillow answers opaque
black where Direct3D specifies zeros."""
import hashlib
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
# per mode: header bits behind the marker (partition, or rotation and index selector), endpoint bits
HEADER = [4, 6, 6, 6, 3, 2, 0, 6]
ENDPOINT_BITS = [72, 72, 90, 84, 42, 58, 56, 80]
RANDOM_FILLS = 4


def pillow_pixels(blocks):
    """(N, 64): Pillow's decoding of the (N, 16) blocks, laid side by side in one 4-pixel-high image"""
    n = blocks.shape[0]
    image = Image.frombytes("RGBA", (4 * n, 4), blocks.tobytes(), "bcn", (7,))
    return np.frombuffer(image.tobytes(), np.uint8).reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 64).copy()


def main():
    rng = np.random.default_rng(0xBC7)
    blocks = []
    for mode in range(8):
        start = mode + 1 + HEADER[mode]
        field = ((1 << ENDPOINT_BITS[mode]) - 1) << start
        for header in range(1 << HEADER[mode]):
            for kind in ["zeros", "ones"] + ["random"] * RANDOM_FILLS:
                v = int.from_bytes(rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), "little")
                v &= ~((1 << start) - 1)
                v |= (1 << mode) | (header << (mode + 1))
                if kind == "zeros":
                    v &= ~field
                elif kind == "ones":
                    v |= field
                blocks.append(np.frombuffer(v.to_bytes(16, "little"), np.uint8))
    blocks = np.stack(blocks)
    assert (blocks[:, 0] != 0).all()
    np.savez_compressed(os.path.join(HERE, "bc7_decode_vectors.npz"), blocks=blocks, pixels=pillow_pixels(blocks))

    payload = open(os.path.join(HERE, "r2-256-bc7.payload.bin"), "rb").read()
    assert len(payload) == 4096 * 16
    image = Image.frombytes("RGBA", (256, 256), payload, "bcn", (7,)).tobytes()
    with open(os.path.join(HERE, "bc7_decode_digests.json"), "w") as f:
        json.dump({"r2-256-bc7.payload.bin": {"width": 256, "height": 256, "sha256": hashlib.sha256(image).hexdigest()}}, f, indent=1)
        f.write("\n")
    print(blocks.shape[0], "blocks")


if __name__ == "__main__":
    main()
