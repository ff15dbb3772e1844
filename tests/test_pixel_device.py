"""The register helpers of the pixel kernels (csrc/pixel_device.h) on the host, through tests/cpp/pixel_device_shim.cpp, against
numpy's uint8 arithmetic: byte-wise add and subtract on four bytes per dword at every byte pair in every slot, the (de)interleave
of sixteen pixels, subtract-green on planes, the 16-byte delta, its prefix sum and the broadcast add at every dword seam.  No
device: the header is plain C++ on dwords and the kernels call these very functions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pixels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAMS = ((3, 4), (7, 8), (11, 12))      # (last byte of a dword, first byte of the next)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "pixel_device_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "pixel_device_shim.cpp")])
    l = C.CDLL(so)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    for name in ("shim_pixel_byte_add", "shim_pixel_byte_sub"):
        getattr(l, name).argtypes, getattr(l, name).restype = [vp, vp, vp, sz], None
    for name in ("shim_pixel_deinterleave", "shim_pixel_interleave"):
        getattr(l, name).argtypes, getattr(l, name).restype = [i, vp, vp, sz], i
    l.shim_pixel_decorrelate_planes.argtypes, l.shim_pixel_decorrelate_planes.restype = [i, i, vp, sz], i
    for name in ("shim_pixel_delta16", "shim_pixel_scan16", "shim_pixel_add_to_all16"):
        getattr(l, name).argtypes, getattr(l, name).restype = [vp, vp, sz], None
    return l


def dwords_op(shim, name, a, b):
    a, b = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(b, dtype=np.uint32)
    out = np.zeros_like(a)
    getattr(shim, name)(a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size)
    return out


def deinterleave(shim, B, px):
    """px: (n, 16, B) bytes -> (n, B, 16)"""
    px = np.ascontiguousarray(px, dtype=np.uint8)
    out = np.zeros((px.shape[0], B, 16), dtype=np.uint8)
    assert shim.shim_pixel_deinterleave(B, px.ctypes.data, out.ctypes.data, px.shape[0]) == 0
    return out


def interleave(shim, B, planes):
    planes = np.ascontiguousarray(planes, dtype=np.uint8)
    out = np.zeros((planes.shape[0], 16, B), dtype=np.uint8)
    assert shim.shim_pixel_interleave(B, planes.ctypes.data, out.ctypes.data, planes.shape[0]) == 0
    return out


def decorrelate(shim, B, inverse, planes):
    p = np.ascontiguousarray(planes, dtype=np.uint8).copy()
    assert shim.shim_pixel_decorrelate_planes(B, int(inverse), p.ctypes.data, p.shape[0]) == 0
    return p


def delta16(shim, vecs, prev):
    p, prev = np.ascontiguousarray(vecs, dtype=np.uint8).copy(), np.ascontiguousarray(prev, dtype=np.uint8)
    assert p.shape == (prev.size, 16)
    shim.shim_pixel_delta16(p.ctypes.data, prev.ctypes.data, prev.size)
    return p


def scan16(shim, vecs):
    p = np.ascontiguousarray(vecs, dtype=np.uint8).copy()
    ret = np.zeros(p.shape[0], dtype=np.uint32)
    shim.shim_pixel_scan16(p.ctypes.data, ret.ctypes.data, p.shape[0])
    return p, ret


def add_to_all16(shim, vecs, x):
    p, x = np.ascontiguousarray(vecs, dtype=np.uint8).copy(), np.ascontiguousarray(x, dtype=np.uint8)
    assert p.shape == (x.size, 16)
    shim.shim_pixel_add_to_all16(p.ctypes.data, x.ctypes.data, x.size)
    return p


def vectors_with_every_pair(rng, lo, hi):
    """65 536 random vectors of 16 bytes in which (byte lo, byte hi) runs through every pair"""
    v = rng.integers(0, 256, (65536, 16), dtype=np.uint8)
    pair = np.arange(65536)
    v[:, lo], v[:, hi] = pair >> 8, pair & 255
    return v


@pytest.mark.parametrize("slot", range(4))
def test_byte_add_and_sub_at_every_byte_pair(shim, slot):
    """All 65 536 (a, b) in byte `slot`; the other three bytes random and different in the two operands, so a carry or borrow that
    crossed a byte boundary in either direction would change a neighbour"""
    rng = np.random.default_rng(0xADD0 + slot)
    pair = np.arange(65536, dtype=np.uint32)
    a8 = rng.integers(0, 256, (65536, 4), dtype=np.uint8)
    b8 = rng.integers(0, 256, (65536, 4), dtype=np.uint8)
    a8[:, slot], b8[:, slot] = pair >> 8, pair & 255
    assert len({(int(x), int(y)) for x, y in zip(a8[:, slot], b8[:, slot])}) == 65536
    others = [k for k in range(4) if k != slot]
    assert (a8[:, others] != b8[:, others]).any(axis=0).all()
    a, b = a8.view("<u4").reshape(-1), b8.view("<u4").reshape(-1)
    assert np.array_equal(dwords_op(shim, "shim_pixel_byte_add", a, b).view(np.uint8).reshape(-1, 4), a8 + b8)
    assert np.array_equal(dwords_op(shim, "shim_pixel_byte_sub", a, b).view(np.uint8).reshape(-1, 4), a8 - b8)


def test_byte_add_and_sub_at_the_extremes(shim):
    """all-ones and all-zero neighbours: the dwords in which a carry out of bit 31 or a borrow below bit 0 would show"""
    vals = np.array([0, 0xFFFFFFFF, 0x80808080, 0x7F7F7F7F, 0x01010101, 0xFF00FF00, 0x00FF00FF, 0x80000000, 0x000000FF], dtype=np.uint32)
    a, b = [x.reshape(-1) for x in np.meshgrid(vals, vals)]
    a8, b8 = a.copy().view(np.uint8).reshape(-1, 4), b.copy().view(np.uint8).reshape(-1, 4)
    assert np.array_equal(dwords_op(shim, "shim_pixel_byte_add", a, b).view(np.uint8).reshape(-1, 4), a8 + b8)
    assert np.array_equal(dwords_op(shim, "shim_pixel_byte_sub", a, b).view(np.uint8).reshape(-1, 4), a8 - b8)


@pytest.mark.parametrize("B", [3, 4])
def test_deinterleave_is_the_transpose_and_interleave_its_inverse(shim, B):
    rng = np.random.default_rng(0xDE1 + B)
    # sixteen pixels of distinct byte values: every byte's destination is told apart; 0..47 / 0..63 is the readable one
    distinct = np.stack([np.arange(16 * B, dtype=np.uint8)] + [rng.permutation(256)[:16 * B].astype(np.uint8) for _ in range(1000)])
    rand = rng.integers(0, 256, (1000, 16 * B), dtype=np.uint8)
    for px in (distinct.reshape(-1, 16, B), rand.reshape(-1, 16, B)):
        planes = deinterleave(shim, B, px)
        assert np.array_equal(planes, px.transpose(0, 2, 1))
        assert np.array_equal(interleave(shim, B, planes), px)
        # and from the planar side: interleave of arbitrary planes, then back
        assert np.array_equal(deinterleave(shim, B, interleave(shim, B, px.reshape(-1, B, 16))), px.reshape(-1, B, 16))
    assert deinterleave(shim, B, distinct[:1].reshape(1, 16, B))[0, 1].tolist() == list(range(1, 16 * B, B))
    assert shim.shim_pixel_deinterleave(5, None, None, 0) == -1


@pytest.mark.parametrize("B", [3, 4])
def test_decorrelate_planes_both_directions(shim, B):
    rng = np.random.default_rng(0xDEC0 + B)
    planes = rng.integers(0, 256, (4096, B, 16), dtype=np.uint8)
    want = planes.copy()
    want[:, 0] -= planes[:, 1]
    want[:, 2] -= planes[:, 1]                      # plane 1 and the alpha plane stay
    fwd = decorrelate(shim, B, False, planes)
    assert np.array_equal(fwd, want)
    assert np.array_equal(decorrelate(shim, B, True, fwd), planes)
    back = planes.copy()
    back[:, 0] += planes[:, 1]
    back[:, 2] += planes[:, 1]
    assert np.array_equal(decorrelate(shim, B, True, planes), back)
    # the chain a lane runs, against the statement of the format: sixteen pixels -> planes -> subtract-green
    px = rng.integers(0, 256, (16, B), dtype=np.uint8)
    lane = decorrelate(shim, B, False, deinterleave(shim, B, px.reshape(1, 16, B)))
    assert np.array_equal(lane.reshape(-1), R.forward(px.reshape(-1), B, True, R.PLANAR))


def delta_cases():
    """(vectors, prev): 10 000 random; every (prev, byte 0) pair; every pair across each of the three dword seams"""
    rng = np.random.default_rng(0xDE17A)
    out = [(rng.integers(0, 256, (10_000, 16), dtype=np.uint8), rng.integers(0, 256, 10_000, dtype=np.uint8))]
    v = rng.integers(0, 256, (65536, 16), dtype=np.uint8)
    pair = np.arange(65536)
    v[:, 0] = pair & 255
    out.append((v, (pair >> 8).astype(np.uint8)))
    for lo, hi in SEAMS:
        out.append((vectors_with_every_pair(rng, lo, hi), rng.integers(0, 256, 65536, dtype=np.uint8)))
    return out


def test_delta16_is_the_difference_with_prev_in_front(shim):
    for vecs, prev in delta_cases():
        want = np.diff(np.concatenate([prev[:, None], vecs], axis=1), axis=1)
        assert want.dtype == np.uint8 and np.array_equal(delta16(shim, vecs, prev), want)


def test_scan16_is_the_running_sum_and_returns_its_last_byte(shim):
    for vecs, prev in delta_cases():
        got, ret = scan16(shim, vecs)
        want = np.cumsum(vecs, axis=1, dtype=np.uint8)
        assert np.array_equal(got, want)
        assert np.array_equal(ret, want[:, 15].astype(np.uint32))      # all 32 bits: nothing above the byte
        assert np.array_equal(scan16(shim, delta16(shim, vecs, np.zeros_like(prev)))[0], vecs)
        # with a byte in front: the scan of the deltas, plus that byte on all sixteen, is the vector again
        assert np.array_equal(add_to_all16(shim, scan16(shim, delta16(shim, vecs, prev))[0], prev), vecs)
    ones = np.full((1, 16), 255, dtype=np.uint8)                       # the carry chain at its longest
    got, ret = scan16(shim, ones)
    assert np.array_equal(got, np.cumsum(ones, axis=1, dtype=np.uint8)) and ret[0] == 0xF0


def test_add_to_all16_at_every_byte(shim):
    rng = np.random.default_rng(0xA11)
    vecs = rng.integers(0, 256, (256 * 64, 16), dtype=np.uint8)
    vecs[:256] = 0xFF
    vecs[256:512] = 0x80
    x = np.tile(np.arange(256, dtype=np.uint8), 64)
    assert np.array_equal(add_to_all16(shim, vecs, x), vecs + x[:, None])
