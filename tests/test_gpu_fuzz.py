"""Seeded random sweep over what a caller can vary at once: format, settings, block count (1 .. ~70 000, biased towards
tile boundaries), the alignment of both device pointers, whole buffer or two ranges of it, and the experiment switches
that select kernel families.  Every case: forward == oracle byte for byte, nothing written outside the output, inverse
gives the source back.  The structured tests cover each axis on its own; this one covers their combinations (it is the
kind of test that caught a store hazard which only showed once a store sat inside an unrolled loop).

`test_random_combinations` draws BC1 / BC2 / BC3; its seed, case count and draw sequence stay as they are so that its history
stays comparable.  BC4 / BC5 and the granule formats (BC6H / BC7) have sweeps of their own beside it, with their own seeds."""
import numpy as np
import pytest

import bc45_ref
import bc6h_ref
import granule_patterns as P
from helpers import BLOCK, all_settings, pkg_settings, settings_id

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = 1500
TILE = {"bc1": 512, "bc2": 256, "bc3": 256, "bc4": 512, "bc5": 256}   # (BC4 / BC5: tests/test_bc45_gpu.py says where from)
IN_OFFSETS = [0, 0, 0, 16, 8, 4, 1, 3]
OUT_OFFSETS = [0, 0, 0, 16, 8, 4, 2, 1, 5]


def pick_count(rng, fmt):
    t = TILE[fmt]
    kind = rng.integers(0, 4)
    if kind == 0:
        return int(rng.integers(1, 70))
    if kind == 1:
        return int(rng.integers(1, 40) * t + rng.integers(-17, 18))
    if kind == 2:
        return int(rng.integers(1, 70_000))
    return int(rng.integers(1, 300) * 16 + rng.integers(0, 2) * rng.integers(0, 16))


def test_random_combinations(pkg, oracle):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0xF0220)
    guard = 64
    try:
        for case in range(CASES):
            fmt = ("bc1", "bc2", "bc3")[int(rng.integers(0, 3))]
            B = BLOCK[fmt]
            settings = list(all_settings(fmt))
            s = settings[int(rng.integers(0, len(settings)))]
            st = pkg_settings(pkg, fmt, s)
            n = max(1, pick_count(rng, fmt))
            in_off = int(rng.choice([0, 0, 0, 16, 8, 4, 1, 3]))
            out_off = int(rng.choice([0, 0, 0, 16, 8, 4, 2, 1, 5]))
            force = int(rng.choice([0, 0, 0, 1, 2, 0x20, 2 | 0x20, 0x100, 0x200]))
            x = rng.integers(0, 256, n * B, dtype=np.uint8)
            want = oracle.transform(fmt, x, s[0], s[2], s[1])
            src = torch.zeros(n * B + 2 * guard, dtype=torch.uint8, device=dev)
            src[in_off:in_off + n * B] = torch.from_numpy(x).to(dev)
            dst = torch.full((n * B + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
            back = torch.full((n * B + 2 * guard,), 0x5A, dtype=torch.uint8, device=dev)
            xin, yout, zout = src[in_off:in_off + n * B], dst[out_off:out_off + n * B], back[in_off:in_off + n * B]
            tag = (case, fmt, settings_id(s), n, in_off, out_off, hex(force))
            pkg.set_tuning(0, force)
            if rng.integers(0, 3) == 0 and n >= 2:
                cut = int(rng.integers(1, n))     # two ranges of one buffer, as a sharded caller issues them
                for first, count in ((0, cut), (cut, n - cut)):
                    pkg.transform_range(fmt, False, xin[first * B:], yout, n, first, count, st)
                for first, count in ((cut, n - cut), (0, cut)):
                    pkg.transform_range(fmt, True, yout, zout[first * B:], n, first, count, st)
            else:
                getattr(pkg, f"transform_{fmt}_with_settings")(xin, yout, st)
                getattr(pkg, f"untransform_{fmt}_with_settings")(yout, zout, st)
            got = dst.cpu().numpy()
            assert np.array_equal(got[out_off:out_off + n * B], want), ("forward",) + tag
            assert (got[:out_off] == 0xA5).all() and (got[out_off + n * B:] == 0xA5).all(), ("forward wrote outside",) + tag
            rt = back.cpu().numpy()
            assert np.array_equal(rt[in_off:in_off + n * B], x), ("inverse",) + tag
            assert (rt[:in_off] == 0x5A).all() and (rt[in_off + n * B:] == 0x5A).all(), ("inverse wrote outside",) + tag
    finally:
        pkg.set_tuning(0, 0)


def guarded_buffers(x, in_off, out_off, dev, guard=64):
    """source at in_off inside a zeroed buffer, output inside 0xA5, round trip inside 0x5A, 2 * guard spare bytes each"""
    nb = x.size
    src = torch.zeros(nb + 2 * guard, dtype=torch.uint8, device=dev)
    src[in_off:in_off + nb] = torch.from_numpy(x).to(dev)
    dst = torch.full((nb + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    back = torch.full((nb + 2 * guard,), 0x5A, dtype=torch.uint8, device=dev)
    return src, dst, back


def check_guarded(dst, back, x, want, in_off, out_off, tag):
    nb = x.size
    got = dst.cpu().numpy()
    assert np.array_equal(got[out_off:out_off + nb], want), ("forward",) + tag
    assert (got[:out_off] == 0xA5).all() and (got[out_off + nb:] == 0xA5).all(), ("forward wrote outside",) + tag
    rt = back.cpu().numpy()
    assert np.array_equal(rt[in_off:in_off + nb], x), ("inverse",) + tag
    assert (rt[:in_off] == 0x5A).all() and (rt[in_off + nb:] == 0x5A).all(), ("inverse wrote outside",) + tag


def test_random_combinations_bc45(pkg):
    """BC4 / BC5: format x endpoint split x count x both pointer offsets x tile lever x whole-or-two-ranges, against
    tests/bc45_ref.py"""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0xF0245)
    try:
        for case in range(1000):
            fmt = ("bc4", "bc5")[int(rng.integers(0, 2))]
            B = bc45_ref.BLOCK[fmt]
            split = bool(rng.integers(0, 2))
            st = (pkg.Bc4TransformSettings if fmt == "bc4" else pkg.Bc5TransformSettings)(split)
            n = max(1, pick_count(rng, fmt))
            in_off, out_off = int(rng.choice(IN_OFFSETS)), int(rng.choice(OUT_OFFSETS))
            force = int(rng.choice([0, 0, 0, 2, 0x20, 0x22]))
            x = rng.integers(0, 256, n * B, dtype=np.uint8)
            want = bc45_ref.transform(fmt, x, split)
            src, dst, back = guarded_buffers(x, in_off, out_off, dev)
            xin, yout, zout = src[in_off:in_off + n * B], dst[out_off:out_off + n * B], back[in_off:in_off + n * B]
            tag = (case, fmt, split, n, in_off, out_off, hex(force))
            pkg.set_tuning(0, force)
            if rng.integers(0, 3) == 0 and n >= 2:
                cut = int(rng.integers(1, n))
                for first, count in ((0, cut), (cut, n - cut)):
                    pkg.transform_range(fmt, False, xin[first * B:], yout, n, first, count, st)
                for first, count in ((cut, n - cut), (0, cut)):
                    pkg.transform_range(fmt, True, yout, zout[first * B:], n, first, count, st)
            else:
                getattr(pkg, f"transform_{fmt}_with_settings")(xin, yout, st)
                getattr(pkg, f"untransform_{fmt}_with_settings")(yout, zout, st)
            check_guarded(dst, back, x, want, in_off, out_off, tag)
    finally:
        pkg.set_tuning(0, 0)


GRANULE_MIXES = ("uniform", "skewed", "raw", "single", "layout")


def granule_blocks(rng, fmt, n, mix):
    """n blocks of BC6H / BC7 under a class mix; "layout": one of the chosen arrangements of tests/granule_patterns.py, tiled"""
    classes = P.CLASSES[fmt]
    if mix == "raw":
        return rng.integers(0, 256, 16 * n, dtype=np.uint8), "raw"
    label = mix
    if mix == "uniform":
        cls = rng.integers(0, classes, n)
    elif mix == "single":
        cls = np.full(n, int(rng.integers(0, classes)), dtype=np.int64)
    elif mix == "skewed":
        few = rng.choice(classes, size=4, replace=False)
        cls = np.where(rng.random(n) < 0.9, few[0], rng.choice(few[1:], size=n))
    else:
        names = P.layout_names(classes)
        label = names[int(rng.integers(0, len(names)))]
        cls = np.resize(P.layout(classes, label), n)
    return P.BLOCKS_WITH_CLASSES[fmt](cls.astype(np.int64), int(rng.integers(0, 1 << 31))), label


def pick_granule_count(rng):
    kind = rng.integers(0, 4)
    if kind == 0:
        return int(rng.integers(1, 71))
    if kind == 3:
        return int(rng.integers(1, 70_000))
    return max(1, int(rng.integers(1, 40) * P.GRANULE + rng.integers(-17, 18)))


def test_random_combinations_granule(pkg, oracle):
    """BC6H / BC7: format x class mix x count (biased to granule boundaries and to tiny tail parts) x both pointer offsets x
    whole-or-two-ranges (cut on a granule: ranges start on one), against tests/bc6h_ref.py and the C statement of BC7"""
    from dxt_lossless_transform_amd import bc6h, bc7

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0xF0267)
    for case in range(600):
        fmt = ("bc6h", "bc7")[int(rng.integers(0, 2))]
        mod = bc7 if fmt == "bc7" else bc6h
        fwd, inv, ranged = (getattr(mod, f"{name}_{fmt}{tail}") for name, tail in (("transform", ""), ("untransform", ""), ("transform", "_range")))
        n = pick_granule_count(rng)
        x, label = granule_blocks(rng, fmt, n, GRANULE_MIXES[int(rng.integers(0, len(GRANULE_MIXES)))])
        in_off, out_off = int(rng.choice(IN_OFFSETS)), int(rng.choice(OUT_OFFSETS))
        want = oracle.transform_bc7(x) if fmt == "bc7" else bc6h_ref.transform(x)
        src, dst, back = guarded_buffers(x, in_off, out_off, dev)
        xin, yout, zout = src[in_off:in_off + 16 * n], dst[out_off:out_off + 16 * n], back[in_off:in_off + 16 * n]
        ranges = bool(rng.integers(0, 3) == 0) and n > P.GRANULE
        tag = (case, fmt, label, n, in_off, out_off, ranges)
        if ranges:
            cut = P.GRANULE * int(rng.integers(1, (n - 1) // P.GRANULE + 1))
            for first, count in ((0, cut), (cut, n - cut)):
                ranged(False, xin[16 * first:], yout, n, first, count)
            for first, count in ((cut, n - cut), (0, cut)):
                ranged(True, yout, zout[16 * first:], n, first, count)
        else:
            fwd(xin, yout)
            inv(yout, zout)
        check_guarded(dst, back, x, want, in_off, out_off, tag)
