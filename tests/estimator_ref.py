"""CPU statement of the built-in size estimator, version 1 of docs/ESTIMATOR.md (TEST INFRASTRUCTURE ONLY: the product has
no CPU implementation).  Two independent statements of the same definition: `estimate` (vectorised numpy, what the tests
use on large inputs) and `estimate_loop` (one position at a time, as the document reads)."""
from __future__ import annotations

import numpy as np

VERSION = 1
W = 32768
BITS = 14
MULT = 2654435761


def _bytes(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def window_matches(b: np.ndarray, bits: int = BITS) -> int:
    """matches of one window (numpy)"""
    n = b.size - 3
    if n <= 0:
        return 0
    g = (b[0:n].astype(np.uint32) | (b[1:n + 1].astype(np.uint32) << 8) | (b[2:n + 2].astype(np.uint32) << 16)
         | (b[3:n + 3].astype(np.uint32) << 24))
    h = ((g.astype(np.uint64) * MULT) & 0xFFFFFFFF) >> (32 - bits)
    _, first_of_slot, inverse = np.unique(h, return_index=True, return_inverse=True)   # return_index: the FIRST occurrence
    f = first_of_slot[inverse.reshape(-1)]
    return int(np.count_nonzero((f < np.arange(n)) & (g[f] == g)))


def estimate(data, w: int = W, bits: int = BITS) -> int:
    b = _bytes(data)
    return b.size - sum(window_matches(b[o:o + w], bits) for o in range(0, b.size, w))


def estimate_loop(data, w: int = W, bits: int = BITS) -> int:
    b = bytes(_bytes(data))
    matches = 0
    for o in range(0, len(b), w):
        win = b[o:o + w]
        first = {}
        for i in range(len(win) - 3):
            g = int.from_bytes(win[i:i + 4], "little")
            s = ((g * MULT) % (1 << 32)) >> (32 - bits)
            if s not in first:
                first[s] = i                      # positions are visited in ascending order: the smallest
            elif int.from_bytes(win[first[s]:first[s] + 4], "little") == g:
                matches += 1
    return len(b) - matches


# docs/ESTIMATOR.md, "A worked vector": 16 bytes, 13 grams in 9 different slots, positions 4..8 repeat 0..3 and 0 -> 16 - 5
WORKED_VECTOR = bytes([1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 9, 9, 9, 9])
WORKED_ESTIMATE = 11


def colliding_grams(count: int = 4096, seed: int = 7, bits: int = BITS) -> np.ndarray:
    """A buffer of 4-byte grams, laid out 4 bytes apart, in which many DIFFERENT gram values share a slot (found by
    search with the definition above): `count` pairs (a, b), a != b, h(a) == h(b), written a b a b.  A table that keeps
    the first gram of a slot must not count b as a match of a -- and the second a is one."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 32, 40 * count + (1 << bits) * 4, dtype=np.uint64)
    h = ((pool * MULT) & 0xFFFFFFFF) >> (32 - bits)
    by_slot = {}
    pairs = []
    for v, s in zip(pool.tolist(), h.tolist()):
        o = by_slot.get(s)
        if o is None:
            by_slot[s] = v
        elif o != v:
            pairs.append((o, v))
            del by_slot[s]
            if len(pairs) == count:
                break
    assert len(pairs) == count
    out = np.array([x for a, b in pairs for x in (a, b, a, b)], dtype=np.uint32)
    return out.view(np.uint8).copy()
