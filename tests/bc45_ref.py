"""CPU restatement of the BC4 / BC5 layout of docs/BC45_FORMAT.md, for the tests only (numpy, no library).

Stream s holds w_s bytes per block and starts at byte off_s * N (N = blocks), off_s being the byte offset of its first field
inside the block; records inside a stream are in block order; index bytes are copied verbatim.

  BC4  split_endpoints = False: (0, 2, a0 a1) (2, 6, idx)            True: (0, 1, a0) (1, 1, a1) (2, 6, idx)
  BC5  the BC4 streams of the red half (byte offsets 0..7), then those of the green half (byte offsets 8..15)
"""
from __future__ import annotations

import numpy as np

BLOCK = {"bc4": 8, "bc5": 16}
FORMAT_CODE = {"bc4": 4, "bc5": 5}


def streams(fmt: str, split_endpoints: bool) -> list[tuple[int, int]]:
    """[(off, width)] of every stream, in order"""
    half = [(0, 1), (1, 1), (2, 6)] if split_endpoints else [(0, 2), (2, 6)]
    if fmt == "bc4":
        return half
    return half + [(8 + off, w) for off, w in half]


def transform(fmt: str, aos: np.ndarray, split_endpoints: bool) -> np.ndarray:
    B = BLOCK[fmt]
    a = np.asarray(aos, dtype=np.uint8)
    assert a.ndim == 1 and a.size % B == 0
    n = a.size // B
    blocks = a.reshape(n, B)
    out = np.empty_like(a)
    for off, w in streams(fmt, split_endpoints):
        out[off * n:(off + w) * n] = blocks[:, off:off + w].reshape(-1)
    return out


def untransform(fmt: str, soa: np.ndarray, split_endpoints: bool) -> np.ndarray:
    B = BLOCK[fmt]
    s = np.asarray(soa, dtype=np.uint8)
    assert s.ndim == 1 and s.size % B == 0
    n = s.size // B
    blocks = np.empty((n, B), dtype=np.uint8)
    for off, w in streams(fmt, split_endpoints):
        blocks[:, off:off + w] = s[off * n:(off + w) * n].reshape(n, w)
    return blocks.reshape(-1)


def endpoint_sections(fmt: str, n: int) -> list[tuple[int, int]]:
    """[(start, end)] of the bytes the auto transform shows its estimator, in order: BC4 [0, 2N); BC5 [0, 2N), [8N, 10N)"""
    return [(0, 2 * n)] if fmt == "bc4" else [(0, 2 * n), (8 * n, 10 * n)]


def auto_choice(fmt: str, aos: np.ndarray, estimate) -> bool:
    """split_endpoints the auto transform picks with `estimate(bytes) -> size`: candidates False, True, strict `<` against a best
    that starts at "no split" with 2**64 - 1 (transform_auto), so a candidate that answers the maximum never wins"""
    n = aos.size // BLOCK[fmt]
    best, best_size = False, 2**64 - 1
    for cand in (False, True):
        t = transform(fmt, aos, cand)
        size = sum(estimate(t[a:b].tobytes()) for a, b in endpoint_sections(fmt, n))
        if size < best_size:
            best, best_size = cand, size
    return best
