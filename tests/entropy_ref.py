"""CPU statement of the entropy estimator, version 1 of docs/ESTIMATOR.md "The entropy estimator, version 1" (TEST
INFRASTRUCTURE ONLY: the product has no CPU implementation), and of the pixel auto transform's choice with it.

    q(window)  = max(0, n T[n] - sum over byte values v of c[v] T[c[v]])      1/65536 bit, exact integers
    T[k]       = floor(2^16 log2 k), k = 1..32768; T[0] = 0
    estimate   = (sum of q over the section's 32768-byte windows + 2^19 - 1) >> 19

The table is built here from the definition -- math.log2 in double precision, a power of two exact, every other k asserted to lie
more than 1e-6 from an integer so that the floor is certain -- independently of tools/gen_entropy_table.py."""
from __future__ import annotations

import math

import numpy as np

VERSION = 1
W = 32768
SHIFT = 19


def _table():
    t = np.zeros(W + 1, dtype=np.int64)
    for k in range(1, W + 1):
        if k & (k - 1) == 0:
            t[k] = (k.bit_length() - 1) << 16
        else:
            x = 65536.0 * math.log2(k)
            assert 1e-6 < x - math.floor(x) < 1 - 1e-6, k
            t[k] = math.floor(x)
    return t


T = _table()


def _bytes(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def window_cost(b: np.ndarray) -> int:
    """q of one window of at most W bytes"""
    c = np.bincount(b, minlength=256).astype(np.int64)
    return max(0, int(b.size * T[b.size]) - int((c * T[c]).sum()))


def section_cost(data) -> int:
    b = _bytes(data)
    return sum(window_cost(b[o:o + W]) for o in range(0, b.size, W))


def estimate(data) -> int:
    if data is None:
        return 0
    return (section_cost(data) + (1 << SHIFT) - 1) >> SHIFT


# docs/ESTIMATOR.md: the 16-byte vector of the gram estimator
WORKED_VECTOR = bytes([1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 9, 9, 9, 9])
WORKED_COST = 2_423_552
WORKED_ESTIMATE = 5
ANCHORS = {2: 65536, 3: 103872, 32768: 983040}

# ---- the pixel auto transform (include/dxtlt_pixels.h): candidates in the order they are compared ----------------------------------
PLANAR_DELTA, PLANAR, INTERLEAVED = 2, 1, 0
CANDIDATES = [(True, PLANAR_DELTA), (True, PLANAR), (True, INTERLEAVED), (False, PLANAR_DELTA), (False, PLANAR), (False, INTERLEAVED)]


def pick(totals) -> int:
    """the first smallest: from the first candidate with best = UINT64_MAX, replaced on strict `<`"""
    best, at = (1 << 64) - 1, 0
    for i, t in enumerate(totals):
        if t < best:
            best, at = t, i
    return at


def auto(data, pixel_bytes, size_of=estimate):
    """(totals, index of the pick, the pick's output) with `size_of` on every candidate's whole output (tests/pixels_ref.py)"""
    import pixels_ref

    outs = [pixels_ref.forward(data, pixel_bytes, d, l) for d, l in CANDIDATES]
    totals = [int(size_of(o)) for o in outs]
    at = pick(totals)
    return totals, at, outs[at]
