"""tests/wide_common.py on CPU tensors at small sizes: the patterns hold every class, the chunked comparisons accept what is right
and name the first wrong element of what is not -- across chunk boundaries, pitch gaps, guards and a clipped last block row.  The
expected images here are built by numpy in pixel order, not by the helper's own permutation."""
import numpy as np
import pytest
import torch

import wide_common as W

FMTS = ["bc1", "bc2", "bc3", "bc4", "bc5", "bc7", "bc6h"]


def arena(nbytes=1 << 20):
    return W.Arena("cpu", nbytes)


@pytest.mark.parametrize("fmt", FMTS)
def test_patterns_and_their_decodes(oracle, fmt):
    pat = W.pattern_of(fmt)
    assert pat.shape == (W.P, W.BLOCK[fmt]) and not pat.flags.writeable
    assert np.array_equal(pat, W.pattern_of(fmt))   # seeded
    dec = W.decoded_pattern(oracle, fmt, pat)
    assert dec.shape == (W.P, 16 * W.BPP[fmt]) and dec.dtype == np.uint8
    assert len(np.unique(dec, axis=0)) > W.P - 64   # a shifted or repeated block shows


def test_lanes_make_a_second_grid_row_of_four_workgroups():
    assert (W.LANES + 255) // 256 == 2**20 + 4
    assert all(W.P % k for k in (2, 3, 64, 256, 1024, W.WIDE_BLOCKS_PER_ROW)) and W.WIDE_BLOCKS_PER_ROW % W.P


def test_tiled_is_the_pattern_modulo_its_length():
    pat = np.arange(7 * 3, dtype=np.uint8).reshape(7, 3)
    for n, first in ((1, 0), (7, 0), (23, 0), (23, 5), (23, 12)):
        got = W.tiled(pat, n, arena(), first).numpy().reshape(n, 3)
        assert np.array_equal(got, pat[(first + np.arange(n)) % 7])


def test_check_records_finds_one_wrong_byte_in_any_chunk():
    expected = np.random.default_rng(1).integers(0, 256, (11, 8), dtype=np.uint8)
    n = 1000
    out = W.tiled(expected, n, arena())
    W.check_records(out, torch.from_numpy(expected), n, "ok", chunk=8 * 64)
    W.check_records(W.tiled(expected, n, arena(), first=4), torch.from_numpy(expected), n, "ok", first=4, chunk=8 * 64)
    for element, byte in ((0, 0), (63, 7), (64, 0), (999, 3)):
        bad = out.clone()
        bad[8 * element + byte] ^= 1
        with pytest.raises(pytest.fail.Exception, match=rf"first wrong element {element}, byte {byte} of it, byte offset {8 * element + byte}:"):
            W.check_records(bad, torch.from_numpy(expected), n, "bad", chunk=8 * 64)
    with pytest.raises(pytest.fail.Exception, match="first wrong element 0,"):   # an array that is one element late
        W.check_records(W.tiled(expected, n, arena(), first=1), torch.from_numpy(expected), n, "late", chunk=8 * 64)


def numpy_image(expected, first, width, height, bpp, pitch):
    """pixel by pixel: (x, y) is pixel 4 (y % 4) + x % 4 of block (y // 4) * blocks_per_row + x // 4"""
    bpr = (width + 3) // 4
    buf = np.full(pitch * (height - 1) + bpp * width, W.FILL, dtype=np.uint8)
    for y in range(height):
        for x in range(width):
            b = (first + (y // 4) * bpr + x // 4) % expected.shape[0]
            p = 4 * (y % 4) + x % 4
            buf[y * pitch + bpp * x:y * pitch + bpp * (x + 1)] = expected[b, bpp * p:bpp * (p + 1)]
    return buf


@pytest.mark.parametrize("bpp", [1, 2, 4, 8])
def test_check_image_against_a_pixel_by_pixel_image(bpp):
    expected = np.random.default_rng(bpp).integers(0, 256, (13, 16 * bpp), dtype=np.uint8)
    expected[expected == W.FILL] = 0
    width, height = 20, 30                       # 5 x 8 blocks, the last block row clipped to two rows
    pitch = bpp * width + 5
    buf = numpy_image(expected, 3, width, height, bpp, pitch)
    dev_expected = torch.from_numpy(expected)
    for chunk in (W.CHUNK, 4 * pitch, 12 * pitch):   # everything at once, one block row, three block rows at a time
        W.check_image(torch.from_numpy(buf), pitch, width, height, bpp, dev_expected, "ok", first=3, chunk=chunk)
        for x, y in ((0, 0), (19, 3), (7, 4), (19, 28), (0, 29), (19, 29)):
            bad = buf.copy()
            bad[y * pitch + bpp * x + bpp - 1] ^= 0x80
            with pytest.raises(pytest.fail.Exception, match=rf"first wrong pixel \({x}, {y}\), byte offset {y * pitch + bpp * x + bpp - 1}:"):
                W.check_image(torch.from_numpy(bad), pitch, width, height, bpp, dev_expected, "bad", first=3, chunk=chunk)
        for y in (0, 3, 15, 28):                     # a byte between two rows
            bad = buf.copy()
            bad[y * pitch + bpp * width + 2] = 0
            with pytest.raises(AssertionError, match="bytes between the rows"):
                W.check_image(torch.from_numpy(bad), pitch, width, height, bpp, dev_expected, "gap", first=3, chunk=chunk)
    with pytest.raises(pytest.fail.Exception):       # the image of the neighbouring blocks
        W.check_image(torch.from_numpy(buf), pitch, width, height, bpp, dev_expected, "late", first=4)


@pytest.mark.parametrize("width,height", [(20, 9), (18, 9), (20, 2), (9, 5)])
def test_check_small_image_and_the_guards(width, height):
    bpp = 4
    expected = np.random.default_rng(9).integers(0, 256, (15, 64), dtype=np.uint8)
    expected[expected == W.FILL] = 0
    pitch = bpp * width + 12
    buf = numpy_image(expected, 0, width, height, bpp, pitch)
    want = W.small_image_bytes(expected, width, height, bpp)
    assert np.array_equal(want, np.stack([buf[y * pitch:y * pitch + bpp * width] for y in range(height)]))

    def guarded(data):
        return W.Guarded(arena(), data.size, off=4, data=torch.from_numpy(data))

    g = guarded(buf)
    g.check_guards()
    W.check_small_image(g, pitch, width, height, bpp, want, "ok")
    assert W.count_not_fill(g.base) == 0          # and the allocation can be used again
    bad = buf.copy()
    bad[(height - 1) * pitch + bpp * (width - 1)] ^= 1
    with pytest.raises(pytest.fail.Exception, match=rf"first wrong pixel \({width - 1}, {height - 1}\)"):
        W.check_small_image(guarded(bad), pitch, width, height, bpp, want, "bad")
    for at in (0, g.at - 1, g.at + bpp * width, g.at + buf.size, g.base.numel() - 1):   # guards and the gap behind row 0
        g = guarded(buf)
        g.base[at] = 0
        with pytest.raises(AssertionError, match="1 bytes outside the image's rows"):
            W.check_small_image(g, pitch, width, height, bpp, want, "stray")
    g = guarded(buf)
    g.base[g.at + buf.size] = 0
    with pytest.raises(AssertionError, match="1 guard bytes"):
        g.check_guards()


def test_arena_cuts_aligned_arrays_and_skips_what_does_not_fit():
    a = W.Arena("cpu", 8 << 20)
    a.need(1 << 20, "a small case")
    x, y = a.take(1000), a.take(24, off=8)
    assert (x.data_ptr() - a.buf.data_ptr()) % 256 == 0 and (y.data_ptr() - a.buf.data_ptr()) % 256 == 8
    assert y.data_ptr() >= x.data_ptr() + 1000
    g = W.Guarded(a, 100, off=1)
    assert (g.view.data_ptr() - a.buf.data_ptr()) % 256 == 1 and g.base.numel() == 2 * W.GUARD + 101
    a.need(1 << 20, "the next case")       # starts at the front again
    assert a.take(16).data_ptr() == a.buf.data_ptr()
    with pytest.raises(pytest.skip.Exception, match=r"needs 0\.0 GiB for a large case plus 8 GiB"):
        a.need(5 << 20, "a large case")    # 4 MiB of slack are part of every case
    with pytest.raises(AssertionError, match="`need` is too small"):
        a.take(9 << 20)
