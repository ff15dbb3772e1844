"""dxtlt_untransform_decode_bc6h_images_batch_device past its 32-bit edges, on the MI355X (the method: tests/wide_common.py; the
BC7 batch call's cases are in tests/test_wide_offsets_gpu.py): an item whose image lies at a `first_block` whose bytes are beyond
2^32, and an image whose rows lie 2^30 + 48 bytes apart.  Expected values come from the CPU statement over a pattern of 4093
blocks; every comparison is exact, and the bytes between far rows are counted on the device.  A test skips only when the card has
less free memory than it needs plus 8 GiB."""
import numpy as np
import pytest

import wide_common as W

pytestmark = pytest.mark.gpu

P = W.P
NEED = 2 * 16 * (2**28 + 8 * 1024 + 77) + (64 << 20)   # the larger case: the blocks and their transform, 4.1 GiB each


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def arena(dev):
    """every large array of this module, allocated once: wide_common.Arena's rule -- the card's free memory less SPARE -- capped at
    what the larger case needs instead of at the 53 GiB of tests/test_wide_offsets_gpu.py"""
    import torch

    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    a = W.Arena(dev, max(0, min(NEED, free - W.SPARE)))
    a.free = free
    yield a
    a.buf = None
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def decoded(oracle):
    """(the pattern, its decoded records), both (P, ..) numpy"""
    pat = W.pattern_of("bc6h")
    return pat, W.decoded_pattern(oracle, "bc6h", pat)


def on(dev, a):
    import torch

    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)   # (a copy: the patterns are read-only arrays)


def small_out(arena, width, height):
    pitch = 8 * width + 16
    return W.Guarded(arena, pitch * (height - 1) + 8 * width), pitch


def payload(g, pitch, width, height):
    rows = g.view.cpu().numpy()
    return np.stack([rows[y * pitch:y * pitch + 8 * width] for y in range(height)])


def check_small(out, dec, first, width, height, pitch, what):
    """a small image whose block b is decoded pattern block (first + b) % P; spoils the output"""
    count = ((width + 3) // 4) * ((height + 3) // 4)
    want = W.small_image_bytes(dec[(first + np.arange(count)) % P], width, height, 8)
    W.check_small_image(out, pitch, width, height, 8, want, what)


def test_an_item_whose_image_lies_beyond_four_gib_beside_a_small_item(pkg, dev, arena, decoded):
    """2^28 + 8 * 1024 + 77 blocks, tiled and transformed on the device by the library's forward call: in ONE batch call a
    260 x 132 image (2145 blocks, over two granule boundaries) at block 2^28 + 1024 + 517 and a 36 x 10 image in the tail part as
    one item, and a 64 x 64 buffer of its own as a second one.  Each item equals its single call"""
    import bc6h_ref
    from dxt_lossless_transform_amd import bc6h, image

    total = 2**28 + 8 * 1024 + 77
    far, tail = (2**28 + 1024 + 517, 260, 132), (total - 32, 36, 10)
    granule = bc6h.sort_granule()
    assert far[0] * 16 > 2**32 and far[0] // granule + 2 <= (far[0] + 2145 - 1) // granule   # two granule boundaries inside
    assert total - total % granule <= tail[0] and tail[0] + 27 <= total                      # the tail part
    pat, dec = decoded
    arena.need(2 * 16 * total, "bc6h blocks and their transform")
    t = arena.take(16 * total)
    bc6h.transform_bc6h(W.tiled(pat, total, arena), t)
    ts = on(dev, bc6h_ref.transform(np.ascontiguousarray(pat[:256]).reshape(-1)))
    batch = [small_out(arena, w, h) for _, w, h in (far, tail, (0, 64, 64))]
    image.untransform_decode_bc6h_images_batch([
        (t, [far, tail], {"outs": [batch[0][0].view, batch[1][0].view], "pitches": [batch[0][1], batch[1][1]]}),
        (ts, [(0, 64, 64)], {"outs": [batch[2][0].view], "pitches": [batch[2][1]]})])
    alone = [small_out(arena, w, h) for _, w, h in (far, tail, (0, 64, 64))]
    image.untransform_decode_bc6h_images(t, [far, tail], outs=[alone[0][0].view, alone[1][0].view], pitches=[alone[0][1], alone[1][1]])
    image.untransform_decode_bc6h_images(ts, [(0, 64, 64)], outs=[alone[2][0].view], pitches=[alone[2][1]])
    for (first, w, h), (got, pitch), (want, _) in zip((far, tail, (0, 64, 64)), batch, alone):
        assert np.array_equal(payload(got, pitch, w, h), payload(want, pitch, w, h)), f"the batch call and the single call differ at block {first}"
    for (first, w, h), (got, pitch) in zip((far, tail, (0, 64, 64)), batch):
        check_small(got, dec, first, w, h, pitch, f"BC6H batch, the image at block {first}")


def test_an_image_whose_rows_lie_two_to_the_thirty_bytes_apart(pkg, dev, arena, decoded):
    """a 20 x 9 image (5 x 3 blocks, the last block row clipped to one pixel row) whose rows lie 2^30 + 48 bytes apart: the pixels
    against the CPU statement, every other byte of the 8 GiB still 0xA5, counted on the device"""
    import bc6h_ref
    from dxt_lossless_transform_amd import image

    width, height, pitch = 20, 9, 2**30 + 48
    pat, dec = decoded
    count = 5 * ((height + 3) // 4)
    blocks = np.ascontiguousarray(pat[:count])
    want = W.small_image_bytes(dec[:count], width, height, 8)
    nbytes = pitch * (height - 1) + 8 * width
    assert nbytes > 2**32 and nbytes + (4 << 20) <= NEED
    arena.need(nbytes, "the far rows")
    transformed = on(dev, bc6h_ref.transform(blocks.reshape(-1)))
    out = W.Guarded(arena, nbytes)
    image.untransform_decode_bc6h_images_batch([(transformed, [(0, width, height)], {"outs": [out.view], "pitches": [pitch]})])
    W.check_small_image(out, pitch, width, height, 8, want, f"bc6h batch, pitch {pitch}")
