"""Inputs for the granule sort of BC7 and BC6H (csrc/granule_sort.h) whose class arrangement is chosen, not drawn: per-block
class numbers laid out so that the sort's packed counters, wave masks and row-to-segment map see their edge values (a segment
count of 64 next to 0, a class total of 1023 or 1024, a class that lives in one segment, the reserved class alone in a
segment), and builders that turn such an array into blocks of exactly those classes.

A granule is 1024 blocks = 16 segments of 64 consecutive blocks.  The kernels give lane t of a 256-lane workgroup the blocks
t, t + 256, t + 512, t + 768, so segment s is handled by wave s % 4 as its (s // 4)-th segment.

Plain module (no fixtures): tests/test_granule_patterns.py, tests/test_gpu_fuzz.py and tests/test_batch.py import it.
"""
from __future__ import annotations

import numpy as np

import bc6h_ref
from oracle import oracle_np

GRANULE = 1024
SEGMENT = 64
STRANGER_POSITIONS = (0, 63, 64, 255, 256, 959, 960, 1023)
BC6H_RESERVED_CODES = (19, 23, 27, 31)


def _segments(classes_of_segment, granule):
    return np.repeat(np.asarray(classes_of_segment, dtype=np.int64), SEGMENT)[:granule]


def class_layouts(classes: int, granule: int = GRANULE):
    """(name, int64 array of per-block class numbers 0..classes-1), each a whole number of granules except the
    `*_then_tail` ones.  The last class (classes - 1) is the format's reserved one."""
    assert granule % SEGMENT == 0
    segs = granule // SEGMENT
    last = classes - 1
    s = np.arange(segs)
    i = np.arange(granule)
    out = {}

    # counts 64 / 0 side by side, different per segment; the second granule one segment further
    out["segment_pure"] = np.concatenate([_segments(s % classes, granule), _segments((s + 1) % classes, granule)])
    round_robin = i % classes
    out["round_robin"] = round_robin                               # every class in every segment, boundaries inside waves
    out["ascending"] = np.sort(round_robin)                        # the identity permutation
    out["descending"] = np.sort(round_robin)[::-1].copy()          # every block moves
    for p in STRANGER_POSITIONS:
        # the others are of the class that differs from the reserved one in the fourth class bit only (BC7: 0 against 8, BC6H: 6
        # against 14), so a match that loses that bit merges the stranger with its neighbours.  BC7: one segment on the ballot
        # path, fifteen on the scan path
        a = np.full(granule, last - 8, dtype=np.int64)
        a[p] = last
        out[f"one_stranger_p{p}"] = a
        b = np.full(granule, last, dtype=np.int64)
        b[p] = 0
        out[f"reserved_with_stranger_p{p}"] = b
    out["all_reserved"] = np.full(granule, last, dtype=np.int64)
    # class totals of exactly 1023 and 1, the single block in front of and behind the others in sorted order
    a = np.full(granule, 5, dtype=np.int64)
    a[517] = 2
    out["exact_1023_plus_1_sorts_first"] = a
    a = np.full(granule, 2, dtype=np.int64)
    a[64] = 7
    out["exact_1023_plus_1_sorts_last"] = a
    # two classes of 512 each: the kernel adds the 16-bit counts of segments 2k and 2k + 1 as the halves of one dword, so
    # alternating segments put 64 and 0 (then 0 and 64) into every dword of both classes
    out["exact_512_512_even_odd"] = _segments(np.where(s % 2 == 0, 1, 6), granule)
    out["exact_512_512_odd_even"] = _segments(np.where(s % 2 == 0, last, 3), granule)
    # class from the wave that loads the block, and from the segment group (the wave's 16-lane row)
    out["by_wave"] = (2 * ((i // SEGMENT) % 4) + 1) % classes
    out["by_segment_group"] = (last - 2 * (i // (4 * SEGMENT))) % classes
    out["by_wave_and_group"] = ((i // SEGMENT) % 4 + 3 * (i // (4 * SEGMENT))) % classes
    # neighbours must not leak through LDS: different granules back to back, then a tail part
    out["two_granules_differ_then_tail"] = np.concatenate([out["descending"], out["all_reserved"], round_robin[:333]])
    out["stranger_then_halves_then_tail"] = np.concatenate([out["one_stranger_p63"], out["exact_512_512_even_odd"],
                                                            np.full(1, last, dtype=np.int64)])
    out["waves_then_groups_then_tail"] = np.concatenate([out["by_wave"], out["by_segment_group"], out["descending"][:1023]])
    for name, cls in out.items():
        assert cls.dtype == np.int64 and cls.min() >= 0 and cls.max() < classes, name
        assert name.endswith("_then_tail") or cls.size % granule == 0, name
        yield name, cls


def layout_names(classes: int) -> list[str]:
    return [name for name, _ in class_layouts(classes)]


def layout(classes: int, name: str) -> np.ndarray:
    return dict(class_layouts(classes))[name]


def bc7_blocks_with_classes(cls, seed: int) -> np.ndarray:
    """16 bytes per entry of cls: random bits, byte 0 forced to class 0..7 = mode marker `1 << m` under random higher bits,
    class 8 = byte 0 == 0 (the reserved encoding)"""
    cls = np.asarray(cls, dtype=np.int64)
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(cls.size, 16), dtype=np.uint8)
    m = np.minimum(cls, 7)
    keep = b[:, 0].astype(np.int64) & ~((2 << m) - 1) & 0xFF
    b[:, 0] = np.where(cls == 8, 0, keep | (1 << m)).astype(np.uint8)
    assert np.array_equal(oracle_np.bc7_modes(b[:, 0]), cls)
    return b.reshape(-1)


def bc6h_blocks_with_classes(cls, seed: int) -> np.ndarray:
    """16 bytes per entry of cls: random bits, the mode bits of byte 0 forced to bc6h_ref.MODE_BITS[class] for 0..13 and to
    one of the four reserved five-bit codes for class 14"""
    cls = np.asarray(cls, dtype=np.int64)
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(cls.size, 16), dtype=np.uint8)
    codes = np.array(bc6h_ref.MODE_BITS + (0,), dtype=np.int64)[cls]
    codes = np.where(cls == bc6h_ref.RESERVED, rng.choice(BC6H_RESERVED_CODES, size=cls.size), codes)
    mask = np.where(cls <= 1, 3, 0x1F)
    b[:, 0] = ((b[:, 0].astype(np.int64) & ~mask & 0xFF) | codes).astype(np.uint8)
    assert np.array_equal(bc6h_ref.block_class(b[:, 0]), cls)
    return b.reshape(-1)


CLASSES = {"bc7": 9, "bc6h": bc6h_ref.CLASSES}
BLOCKS_WITH_CLASSES = {"bc7": bc7_blocks_with_classes, "bc6h": bc6h_blocks_with_classes}


def blocks_of_layout(fmt: str, name: str, seed: int = 0) -> np.ndarray:
    return BLOCKS_WITH_CLASSES[fmt](layout(CLASSES[fmt], name), seed)


def all_layouts_then_tail(fmt: str, tail: int, seed: int = 0):
    """every whole-granule layout back to back (tens of granules), then `tail` round-robin blocks: (classes, blocks)"""
    classes = CLASSES[fmt]
    parts = [cls for name, cls in class_layouts(classes) if not name.endswith("_then_tail")]
    parts.append(np.arange(tail, dtype=np.int64) % classes)
    cls = np.concatenate(parts)
    return cls, BLOCKS_WITH_CLASSES[fmt](cls, seed)


def tail_classes(fmt: str, n: int) -> np.ndarray | None:
    """classes of an n-block buffer of the every-tail-length sweeps: round robin for odd n, None (= raw random bytes, whatever
    classes they have) for even n"""
    return np.arange(n, dtype=np.int64) % CLASSES[fmt] if n % 2 else None


def tail_blocks(fmt: str, n: int, rng) -> np.ndarray:
    cls = tail_classes(fmt, n)
    if cls is None:
        return rng.integers(0, 256, 16 * n, dtype=np.uint8)
    return BLOCKS_WITH_CLASSES[fmt](cls, int(rng.integers(0, 1 << 31)))
