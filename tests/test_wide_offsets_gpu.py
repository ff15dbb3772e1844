"""The element-wise and image kernels past their 32-bit edges, on the MI355X (the method: tests/wide_common.py).

Every kernel here takes its element number from workgroup_index() * threads + threadIdx.x (csrc/launch_grid.h) and scales it to
byte offsets in code of its own.  grid_rows() starts a second grid row at 2^28 lanes, so every case of part A runs
k * (2^28 + 3 * 256 + 77) elements for a kernel of k elements per lane: 2^20 + 4 workgroups, a full first row and four workgroups
of the second, outputs -- and, at 16 bytes per lane, inputs -- that cross byte 2^32.  Part B runs the fused image calls on a
`first_block` whose bytes lie beyond 2^32, part C every image sink on a pixel offset beyond 2^32 (a small image with a far pitch).
Expected values come from the CPU statements over a pattern of 4093 blocks, or, for the pixel transform, from a few torch lines
after docs/PIXEL_FORMAT.md; every comparison is exact and runs on the device.  A test skips only when the card has less free
memory than it needs plus 8 GiB."""
import functools

import numpy as np
import pytest

import wide_common as W

pytestmark = pytest.mark.gpu

P, LANES = W.P, W.LANES


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def arena(dev):
    """every large array of this module: allocated once (wide_common.Arena has the reason), given back at the end"""
    import torch

    a = W.Arena(dev)
    yield a
    a.buf = None
    torch.cuda.empty_cache()


_decoded = {}


def decoded(oracle, fmt):
    """(pattern, its decoded records), both (P, ..) numpy, computed once"""
    if fmt not in _decoded:
        pat = W.pattern_of(fmt)
        _decoded[fmt] = (pat, W.decoded_pattern(oracle, fmt, pat))
    return _decoded[fmt]


def on(dev, a):
    import torch

    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)   # (a copy: the patterns are read-only arrays)


# =========================================================================================================================
# A.1 / A.2: the block decoders
# =========================================================================================================================
def run_block_decoder(arena, call, pat, dec, n, what, off=0):
    bs, rec = pat.shape[1], dec.shape[1]
    arena.need(n * bs + n * rec, what)
    src = W.tiled(pat, n, arena, off=off)
    out = W.Guarded(arena, rec * n, off)
    call(src, out.view)
    W.check_records(out.view, on(arena.device, dec), n, what)
    out.check_guards()


@pytest.mark.parametrize("fmt", ["bc1", "bc2", "bc3"])
def test_decode_blocks_in_the_second_grid_row(pkg, oracle, dev, arena, fmt):
    from dxt_lossless_transform_amd import decode

    pat, dec = decoded(oracle, fmt)
    run_block_decoder(arena, functools.partial(decode.decode_blocks, fmt), pat, dec, LANES, f"decode_blocks {fmt}")


def test_decode_blocks_bc1_unaligned_in_the_second_grid_row(pkg, oracle, dev, arena):
    """both pointers 1 byte off: the byte-load, byte-store kernel (64 * b bytes in its own arithmetic)"""
    from dxt_lossless_transform_amd import decode

    pat, dec = decoded(oracle, "bc1")
    run_block_decoder(arena, functools.partial(decode.decode_blocks, "bc1"), pat, dec, LANES, "decode_blocks bc1, unaligned", off=1)


def test_decode_bc7_blocks_in_the_second_grid_row(pkg, oracle, dev, arena):
    from dxt_lossless_transform_amd import decode

    pat, dec = decoded(oracle, "bc7")
    run_block_decoder(arena, decode.decode_bc7_blocks, pat, dec, LANES, "decode_bc7_blocks")


def test_decode_bc6h_blocks_in_the_second_grid_row(pkg, oracle, dev, arena):
    """the largest case: 4 GiB of blocks, 32 GiB of pixels"""
    from dxt_lossless_transform_amd import decode

    pat, dec = decoded(oracle, "bc6h")
    run_block_decoder(arena, decode.decode_bc6h_blocks, pat, dec, LANES, "decode_bc6h_blocks")


def test_count_pixel_differences_beyond_four_gib(pkg, oracle, dev, arena):
    """two arrays of 2 * LANES + 1 BC1 blocks (the kernel takes two blocks per lane and step; 4 GiB each) that differ in every
    1021st block and in the last: every third of those differs in its bytes but not in its pixels (equal endpoints, other
    indices), so the count is the closed form below"""
    import torch
    from dxt_lossless_transform_amd import decode

    n = 2 * LANES + 1
    same_a = np.array([0x34, 0x12, 0x34, 0x12, 0x00, 0x00, 0x00, 0x00], dtype=np.uint8)   # c0 == c1: indices 0 and 1 are one colour
    same_b = np.array([0x34, 0x12, 0x34, 0x12, 0x55, 0x55, 0x55, 0x55], dtype=np.uint8)
    diff_a = np.array([0x00, 0xF8, 0x1F, 0x00, 0x00, 0x00, 0x00, 0x00], dtype=np.uint8)   # red
    diff_b = np.array([0xE0, 0x07, 0x1F, 0x00, 0x00, 0x00, 0x00, 0x00], dtype=np.uint8)   # green
    assert oracle.count_pixel_differences("bc1", same_a, same_b) == 0 and not np.array_equal(same_a, same_b)
    assert oracle.count_pixel_differences("bc1", diff_a, diff_b) == 1
    arena.need(2 * 8 * n, "two BC1 arrays")
    pat, _ = decoded(oracle, "bc1")
    a = W.tiled(pat, n, arena)
    b = arena.take(8 * n)
    b.copy_(a)
    assert decode.count_pixel_differences("bc1", a, b) == 0
    a8, b8 = a.view(n, 8), b.view(n, 8)
    at = torch.arange(0, n, 1021, device=dev)
    count = at.numel()
    assert count == (n - 1) // 1021 + 1
    same = at[0::3]
    differ = torch.cat([at[1::3], at[2::3]])
    a8[same], b8[same] = on(dev, same_a), on(dev, same_b)
    a8[differ], b8[differ] = on(dev, diff_a), on(dev, diff_b)
    a8[n - 1], b8[n - 1] = on(dev, diff_a), on(dev, diff_b)
    want = count - (count + 2) // 3      # positions 1, 2 mod 3 of the 1021st blocks
    if (n - 1) % 1021 != 0 or ((n - 1) // 1021) % 3 == 0:
        want += 1                        # the last block is no 1021st one, or was a same-pixels one until it was overwritten
    assert decode.count_pixel_differences("bc1", a, b) == want
    assert decode.count_pixel_differences("bc1", b, a) == want


# =========================================================================================================================
# A.3: normalisation
# =========================================================================================================================
SOLID = (0x00, 0x55, 0xAA, 0xFF)


@functools.lru_cache(maxsize=None)
def normalisable_pattern(fmt):
    """the BC1..BC3 pattern with every fourth block of one colour index (the four values in turn) and, for BC2 / BC3, every
    fourth block of one alpha value (opaque in half of them)"""
    x = np.array(W.bcn_pattern(fmt, seed=3))
    at = 4 if fmt == "bc1" else 12
    for k, v in enumerate(SOLID):
        x[1 + 4 * k::16, at:at + 4] = v
    if fmt == "bc2":
        x[2::8, :8] = 0xFF
        x[6::8, :8] = 0x77
    if fmt == "bc3":
        x[2::8, 0] = x[2::8, 1] = 0xFF
        x[6::8, 1] = x[6::8, 0]
        x[10::16, 2:8] = 0
    x.setflags(write=False)
    return x


def changed_blocks(before, after):
    return int((np.asarray(before).reshape(P, -1) != np.asarray(after).reshape(P, -1)).any(axis=1).sum())


def run_normalize(arena, call, pat, want, n, what, off=0):
    bs = pat.shape[1]
    arena.need(2 * n * bs, what)
    src = W.tiled(pat, n, arena, off=off)
    out = W.Guarded(arena, bs * n, off)
    call(src, out.view)
    W.check_records(out.view, on(arena.device, want.reshape(P, bs)), n, what)
    out.check_guards()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_normalize_bc1_blocks_vector_path(pkg, oracle, dev, arena, mode):
    """two blocks per lane and a ragged last block: 2 * LANES + 1 blocks, 4 GiB in and out"""
    from dxt_lossless_transform_amd import normalize

    pat = normalisable_pattern("bc1")
    want = oracle.normalize_bc1_blocks(pat.reshape(-1), mode)
    assert (0 < changed_blocks(pat, want) < P) if mode else changed_blocks(pat, want) == 0
    run_normalize(arena, lambda s, d: normalize.normalize_blocks(s, d, normalize.ColorNormalizationMode(mode)), pat, want,
                  2 * LANES + 1, f"normalize_blocks bc1 mode {mode}")


def test_normalize_bc1_blocks_singles_path(pkg, oracle, dev, arena):
    """pointers 8 bytes off a 16-byte boundary: one block per lane"""
    from dxt_lossless_transform_amd import normalize

    pat = normalisable_pattern("bc1")
    want = oracle.normalize_bc1_blocks(pat.reshape(-1), 2)
    run_normalize(arena, lambda s, d: normalize.normalize_blocks(s, d, normalize.ColorNormalizationMode.REPLICATE_COLOR), pat, want,
                  LANES, "normalize_blocks bc1 mode 2, singles", off=8)


def test_normalize_bc1_blocks_all_modes(pkg, oracle, dev, arena):
    from dxt_lossless_transform_amd import normalize

    n = 2 * LANES + 1
    pat = normalisable_pattern("bc1")
    wants, any_normalised = oracle.normalize_bc1_blocks_all_modes(pat.reshape(-1))
    assert any_normalised and changed_blocks(wants[1], wants[2]) > 0
    arena.need(4 * 8 * n, "BC1 blocks and three outputs")
    src = W.tiled(pat, n, arena)
    outs = [W.Guarded(arena, 8 * n) for _ in range(3)]
    assert normalize.normalize_blocks_all_modes(src, [o.view for o in outs]) is True
    for mode, (o, want) in enumerate(zip(outs, wants)):
        W.check_records(o.view, on(dev, want.reshape(P, 8)), n, f"normalize_blocks_all_modes bc1, output {mode}")
        o.check_guards()


def test_normalize_bc1_split_blocks_in_place(pkg, oracle, dev, arena):
    """four blocks per lane and a ragged last one: 4 * LANES + 1 blocks, the colour and the index stream 4 GiB each"""
    from dxt_lossless_transform_amd import normalize

    n = 4 * LANES + 1
    pat = normalisable_pattern("bc1")
    colours, indices = np.ascontiguousarray(pat[:, :4]), np.ascontiguousarray(pat[:, 4:])
    want_c, want_i = oracle.normalize_bc1_split_blocks(colours.reshape(-1), indices.reshape(-1), 2)
    assert changed_blocks(colours, want_c) + changed_blocks(indices, want_i) > 0
    arena.need(2 * 4 * n, "the two streams")
    c, i = W.Guarded(arena, 4 * n), W.Guarded(arena, 4 * n)
    W.tiled(colours, n, arena, out=c.view)
    W.tiled(indices, n, arena, out=i.view)
    normalize.normalize_split_blocks_in_place(c.view, i.view, normalize.ColorNormalizationMode.REPLICATE_COLOR)
    W.check_records(c.view, on(dev, want_c.reshape(P, 4)), n, "normalize_split_blocks_in_place, colours")
    W.check_records(i.view, on(dev, want_i.reshape(P, 4)), n, "normalize_split_blocks_in_place, indices")
    c.check_guards()
    i.check_guards()


@pytest.mark.parametrize("fmt,alpha_mode,colour_mode", [("bc2", 0, 1), ("bc3", 1, 2)])
def test_normalize_bc23_blocks(pkg, oracle, dev, arena, fmt, alpha_mode, colour_mode):
    """one block per lane: LANES blocks, 4 GiB in and out"""
    from dxt_lossless_transform_amd import normalize23

    pat = normalisable_pattern(fmt)
    want = (oracle.normalize_bc2_blocks(pat.reshape(-1), colour_mode) if fmt == "bc2"
            else oracle.normalize_bc3_blocks(pat.reshape(-1), alpha_mode, colour_mode))
    assert 0 < changed_blocks(pat, want) < P
    if fmt == "bc3":   # both halves of the mode do something here
        assert changed_blocks(want, oracle.normalize_bc3_blocks(pat.reshape(-1), 0, colour_mode)) > 0
        assert changed_blocks(want, oracle.normalize_bc3_blocks(pat.reshape(-1), alpha_mode, 0)) > 0
    run_normalize(arena, lambda s, d: normalize23.normalize_blocks(fmt, s, d, normalize23.ColorNormalizationMode(colour_mode),
                                                                normalize23.AlphaNormalizationMode(alpha_mode)),
                  pat, want, LANES, f"normalize_blocks {fmt} alpha {alpha_mode} colour {colour_mode}")


@pytest.mark.parametrize("fmt", ["bc2", "bc3"])
def test_normalize_bc23_blocks_all_modes(pkg, oracle, dev, arena, fmt):
    """3 (BC2) or 12 (BC3) outputs of 4 GiB from one read"""
    from dxt_lossless_transform_amd import normalize23

    n = LANES
    pat = normalisable_pattern(fmt)
    wants = oracle.normalize_bc2_blocks_all_modes(pat.reshape(-1)) if fmt == "bc2" else oracle.normalize_bc3_blocks_all_modes(pat.reshape(-1))
    assert len({w.tobytes() for w in wants}) == len(wants)   # no two modes give the same bytes on this pattern
    arena.need((1 + len(wants)) * 16 * n, f"{fmt} blocks and {len(wants)} outputs")
    src = W.tiled(pat, n, arena)
    outs = [W.Guarded(arena, 16 * n) for _ in wants]
    normalize23.normalize_blocks_all_modes(fmt, src, [o.view for o in outs])
    for k, (o, want) in enumerate(zip(outs, wants)):
        W.check_records(o.view, on(dev, want.reshape(P, 16)), n, f"normalize_blocks_all_modes {fmt}, output {k}")
        o.check_guards()


# =========================================================================================================================
# A.4: the colour-array operations, variant 2
# =========================================================================================================================
@functools.lru_cache(maxsize=None)
def colour_table(oracle, inverse):
    f = oracle.recorrelate if inverse else oracle.decorrelate
    return np.array([f(c, 2) for c in range(65536)], dtype="<u2")


def colour_pattern(width, seed):
    x = np.random.default_rng(0xC565 + seed).integers(0, 256, (P, width), dtype=np.uint8)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("inverse", [False, True])
def test_ycocg_arrays_vector_path(pkg, oracle, dev, arena, inverse):
    """ycocg_array_kernel: EIGHT colours (16 bytes) per lane, then one colour per lane: 8 * LANES + 3 colours, 4 GiB in and out"""
    from dxt_lossless_transform_amd import color565

    pat = colour_pattern(16, 1)
    want = np.ascontiguousarray(colour_table(oracle, inverse)[pat.view("<u2")]).view(np.uint8).reshape(P, 16)
    assert changed_blocks(pat, want) == P
    arena.need(2 * 16 * (LANES + 1), "colours in and out")
    nbytes = 16 * LANES + 2 * 3
    src = W.tiled(pat, LANES + 1, arena)[:nbytes]
    out = W.Guarded(arena, nbytes)
    (color565.recorrelate_ycocg_r if inverse else color565.decorrelate_ycocg_r)(src, out.view, 2)
    what = "recorrelate_ycocg_r" if inverse else "decorrelate_ycocg_r"
    W.check_records(out.view[:16 * LANES], on(dev, want), LANES, what)
    assert out.view[16 * LANES:].cpu().numpy().tolist() == want[LANES % P, :6].tolist(), f"{what}: the last three colours"
    out.check_guards()


def test_recorrelate_ycocg_split_vector_path(pkg, oracle, dev, arena):
    """recorrelate_split_kernel: FOUR pairs per lane (8 bytes of each source, 16 of the destination), then one pair per lane:
    4 * LANES + 1 pairs, 4 GiB out"""
    from dxt_lossless_transform_amd import color565

    p0, p1 = colour_pattern(8, 2), colour_pattern(8, 3)
    zipped = np.stack([p0.view("<u2"), p1.view("<u2")], axis=2)            # (P, 4 pairs, c0 c1)
    want = np.ascontiguousarray(colour_table(oracle, True)[zipped]).view(np.uint8).reshape(P, 16)
    arena.need(2 * 16 * (LANES + 1), "two sources and the destination")
    pairs = 4 * LANES + 1
    s0, s1 = W.tiled(p0, LANES + 1, arena)[:2 * pairs], W.tiled(p1, LANES + 1, arena)[:2 * pairs]
    out = W.Guarded(arena, 4 * pairs)
    color565.recorrelate_ycocg_r_split(s0, s1, out.view, 2)
    W.check_records(out.view[:16 * LANES], on(dev, want), LANES, "recorrelate_ycocg_r_split")
    assert out.view[16 * LANES:].cpu().numpy().tolist() == want[LANES % P, :4].tolist(), "recorrelate_ycocg_r_split: the last pair"
    out.check_guards()


def test_split_color_endpoints_vector_path(pkg, oracle, dev, arena):
    """split_endpoints_kernel: EIGHT pairs (32 bytes) per lane; the vector path needs a multiple of eight pairs: 8 * LANES pairs,
    8 GiB in and out, the second half of the output starts beyond byte 2^32"""
    from dxt_lossless_transform_amd import color565

    pat = colour_pattern(32, 4)
    want = np.stack([oracle.split_565_color_endpoints(row) for row in pat])   # per row: sixteen bytes of c0, sixteen of c1
    arena.need(2 * 32 * LANES, "pairs in and out")
    src = W.tiled(pat, LANES, arena)
    out = W.Guarded(arena, 32 * LANES)
    color565.split_color_endpoints(src, out.view)
    W.check_records(out.view[:16 * LANES], on(dev, want[:, :16]), LANES, "split_color_endpoints, c0")
    W.check_records(out.view[16 * LANES:], on(dev, want[:, 16:]), LANES, "split_color_endpoints, c1")
    out.check_guards()


# =========================================================================================================================
# A.5: the plain image decoders into one wide image
# =========================================================================================================================
WIDE_WIDTH = 4 * W.WIDE_BLOCKS_PER_ROW


def wide_image(fmt, blocks):
    """(height, pitch, bytes of the image) of the narrowest-height image of WIDE_WIDTH pixels with `blocks` blocks or more whose
    last block row is clipped to two pixel rows"""
    block_rows = (blocks + W.WIDE_BLOCKS_PER_ROW - 1) // W.WIDE_BLOCKS_PER_ROW
    height = 4 * block_rows - 2
    row_bytes = W.BPP[fmt] * WIDE_WIDTH
    pitch = (row_bytes + 15) // 16 * 16 + 16
    return height, pitch, pitch * (height - 1) + row_bytes


def plain_image_call(fmt):
    from dxt_lossless_transform_amd import image

    if fmt in ("bc1", "bc2", "bc3"):
        return functools.partial(image.decode_image, fmt)
    if fmt in ("bc4", "bc5"):
        return functools.partial(image.decode_channel_image, fmt)
    return image.decode_bc7_image if fmt == "bc7" else image.decode_bc6h_image


@pytest.mark.parametrize("fmt", ["bc1", "bc3", "bc4", "bc5", "bc7", "bc6h"])
def test_plain_image_decoder_in_the_second_grid_row(pkg, oracle, dev, arena, fmt):
    """one image of 65644 pixels' width (16411 blocks per row, a prime) and LANES blocks or more -- twice that for BC4, whose lanes
    take two blocks -- with a padded pitch and a clipped last block row"""
    pat, dec = decoded(oracle, fmt)
    per_lane = 2 if fmt == "bc4" else 1
    height, pitch, nbytes = wide_image(fmt, per_lane * LANES)
    assert height % 4 == 2
    blocks = W.WIDE_BLOCKS_PER_ROW * ((height + 3) // 4)
    assert blocks >= per_lane * LANES and (blocks + per_lane - 1) // per_lane > 2**28   # the grid has its second row
    arena.need(blocks * W.BLOCK[fmt] + nbytes, f"{fmt} blocks and their image")
    src = W.tiled(pat, blocks, arena)
    out = W.Guarded(arena, nbytes)
    plain_image_call(fmt)(src, WIDE_WIDTH, height, out=out.view, pitch=pitch)
    W.check_image(out.view, pitch, WIDE_WIDTH, height, W.BPP[fmt], on(dev, dec), f"plain image decoder {fmt}")
    out.check_guards()


# =========================================================================================================================
# A.6: the region decoders of block arrays
# =========================================================================================================================
def plain_regions_call(fmt):
    from dxt_lossless_transform_amd import image

    if fmt == "bc7":
        return image.decode_bc7_images
    if fmt == "bc6h":
        return image.decode_bc6h_images
    return functools.partial(image.decode_images, fmt)


def small_pitch(fmt, width):
    return W.BPP[fmt] * width + 16


def check_small(dev_out, fmt, dec, first, width, height, pitch, what):
    """a small image whose block b is decoded pattern block (first + b) % P"""
    count = ((width + 3) // 4) * ((height + 3) // 4)
    want = W.small_image_bytes(dec[(first + np.arange(count)) % P], width, height, W.BPP[fmt])
    W.check_small_image(dev_out, pitch, width, height, W.BPP[fmt], want, what)


@pytest.mark.parametrize("fmt", ["bc1", "bc4", "bc7", "bc6h"])
def test_region_decoder_in_the_second_grid_row(pkg, oracle, dev, arena, fmt):
    """three regions of one block array: a wide image of more than LANES blocks (twice that for BC4), a gap of 37 blocks, a 64 x 64
    image, a gap of 11 blocks and a 9 x 5 image that ends at the array's last block: the last two lie in the second grid row"""
    pat, dec = decoded(oracle, fmt)
    per_lane, bpp = (2 if fmt == "bc4" else 1), W.BPP[fmt]
    height0, pitch0, nbytes0 = wide_image(fmt, per_lane * LANES)
    blocks0 = W.WIDE_BLOCKS_PER_ROW * ((height0 + 3) // 4)
    first1 = blocks0 + 37
    first2 = first1 + 256 + 11
    total = first2 + 6
    assert blocks0 // per_lane >= 2**28
    regions = [(0, WIDE_WIDTH, height0), (first1, 64, 64), (first2, 9, 5)]
    pitches = [pitch0, small_pitch(fmt, 64), small_pitch(fmt, 9)]
    arena.need(total * W.BLOCK[fmt] + nbytes0, f"{fmt} blocks and their images")
    src = W.tiled(pat, total, arena)
    outs = [W.Guarded(arena, nbytes0), W.Guarded(arena, pitches[1] * 63 + bpp * 64), W.Guarded(arena, pitches[2] * 4 + bpp * 9)]
    plain_regions_call(fmt)(src, regions, outs=[o.view for o in outs], pitches=pitches)
    W.check_image(outs[0].view, pitch0, WIDE_WIDTH, height0, bpp, on(dev, dec), f"region decoder {fmt}, region 0")
    outs[0].check_guards()
    check_small(outs[1], fmt, dec, first1, 64, 64, pitches[1], f"region decoder {fmt}, region 1")
    check_small(outs[2], fmt, dec, first2, 9, 5, pitches[2], f"region decoder {fmt}, region 2")


# =========================================================================================================================
# A.7: the pixel transforms
# =========================================================================================================================
PIXELS = 2**30 + 4096 + 123
SEGMENT = 4096
PIXEL_CHUNK = 2**26   # pixels per step of the torch statement: a multiple of SEGMENT


def torch_forward(px, decorrelate, planar_delta):
    """docs/PIXEL_FORMAT.md for the pixels `px` (n, B), n starting on a segment boundary: the B planes (B, n), or the pixels
    themselves for the interleaved layout"""
    px = px.clone()
    if decorrelate:
        px[:, 0] -= px[:, 1]      # uint8 arithmetic wraps modulo 256
        px[:, 2] -= px[:, 1]
    if not planar_delta:
        return px
    planes = px.t().contiguous()
    out = planes.clone()
    out[:, 1:] -= planes[:, :-1]
    out[:, ::SEGMENT] = planes[:, ::SEGMENT]   # the first byte of every segment is stored as it is
    return out


@pytest.mark.parametrize("B", [4, 3])
@pytest.mark.parametrize("decorrelate,planar_delta", [(True, True), (False, False)])
def test_pixel_transforms_beyond_two_to_the_thirty_pixels(pkg, dev, arena, B, decorrelate, planar_delta):
    """2^30 + 4096 + 123 pixels: the plane bases c * P and the interleaved offsets B * i both pass 2^32"""
    import pixels_ref
    import torch
    from dxt_lossless_transform_amd import pixels

    layout = pixels.PLANAR_DELTA if planar_delta else pixels.INTERLEAVED
    n = PIXELS
    arena.need(3 * B * n, "pixels, transformed and restored")
    pat = np.random.default_rng(0x9185 + B).integers(0, 256, (P, B), dtype=np.uint8)
    src = W.tiled(pat, n, arena)
    # the torch statement is the numpy statement: on the first three tiles and on the last three (two whole, one of 123 pixels)
    for lo, hi in ((0, 3 * SEGMENT), ((n // SEGMENT - 2) * SEGMENT, n)):
        mine = torch_forward(src[B * lo:B * hi].view(-1, B), decorrelate, planar_delta).cpu().numpy().reshape(-1)
        assert np.array_equal(mine, pixels_ref.forward(src[B * lo:B * hi].cpu().numpy(), B, decorrelate, layout)), (lo, hi)
    out = W.Guarded(arena, B * n)
    pixels.transform_pixels(src, out.view, B, decorrelate, layout)
    for lo in range(0, n, PIXEL_CHUNK):
        hi = min(n, lo + PIXEL_CHUNK)
        want = torch_forward(src[B * lo:B * hi].view(-1, B), decorrelate, planar_delta)
        if planar_delta:
            for c in range(B):
                got = out.view[c * n + lo:c * n + hi]
                if not torch.equal(got, want[c]):
                    i = int(torch.nonzero(got != want[c])[0])
                    pytest.fail(f"transform_pixels B = {B}: plane {c}, first wrong pixel {lo + i}, byte offset {c * n + lo + i}")
        else:
            got = out.view[B * lo:B * hi]
            if not torch.equal(got, want.reshape(-1)):
                i = int(torch.nonzero(got != want.reshape(-1))[0])
                pytest.fail(f"transform_pixels B = {B}: first wrong byte offset {B * lo + i}")
        del want
    out.check_guards()
    back = W.Guarded(arena, B * n)
    pixels.untransform_pixels(out.view, back.view, B, decorrelate, layout)
    for lo in range(0, B * n, W.CHUNK):
        if not torch.equal(back.view[lo:lo + W.CHUNK], src[lo:lo + W.CHUNK]):
            i = int(torch.nonzero(back.view[lo:lo + W.CHUNK] != src[lo:lo + W.CHUNK])[0])
            pytest.fail(f"untransform_pixels B = {B}: first wrong byte offset {lo + i}")
    back.check_guards()


# =========================================================================================================================
# B: the fused image calls at a first_block beyond byte 2^32
# =========================================================================================================================
def small_out(arena, fmt, width, height, pitch=None):
    pitch = small_pitch(fmt, width) if pitch is None else pitch
    return W.Guarded(arena, pitch * (height - 1) + W.BPP[fmt] * width), pitch


def payload(g, pitch, width, height, bpp):
    """the image's rows as one host array, for the "equals the single call" checks"""
    rows = g.view.cpu().numpy()
    return np.stack([rows[y * pitch:y * pitch + bpp * width] for y in range(height)])


@pytest.mark.parametrize("fmt", ["bc7", "bc6h"])
def test_fused_granule_image_calls_beyond_four_gib(pkg, oracle, dev, arena, fmt):
    """2^28 + 8 * 1024 + 77 blocks, tiled and transformed on the device by the library's forward call (pinned at this size by
    tests/test_bc7.py and tests/test_bc6h_gpu.py): a 260 x 132 image (2145 blocks, over two granule boundaries) at block 2^28 +
    1024 + 517, a 36 x 10 image in the tail part, both again in one region call, and (BC7) in one batch call next to a small
    buffer"""
    from dxt_lossless_transform_amd import bc6h, bc7, image

    total = 2**28 + 8 * 1024 + 77
    far, tail = (2**28 + 1024 + 517, 260, 132), (total - 32, 36, 10)
    granule = (bc7 if fmt == "bc7" else bc6h).sort_granule()
    assert far[0] * 16 > 2**32 and far[0] // granule + 2 <= (far[0] + 2145 - 1) // granule   # two granule boundaries inside
    assert total - total % granule <= tail[0] and tail[0] + 27 <= total                      # the tail part
    pat, dec = decoded(oracle, fmt)
    arena.need(2 * 16 * total, f"{fmt} blocks and their transform")
    t = arena.take(16 * total)
    (bc7.transform_bc7 if fmt == "bc7" else bc6h.transform_bc6h)(W.tiled(pat, total, arena), t)
    single = image.untransform_decode_bc7_image if fmt == "bc7" else image.untransform_decode_bc6h_image
    regions_call = image.untransform_decode_bc7_images if fmt == "bc7" else image.untransform_decode_bc6h_images
    bpp, kept = W.BPP[fmt], []
    for first, width, height in (far, tail):
        out, pitch = small_out(arena, fmt, width, height)
        single(t, width, height, first_block=first, out=out.view, pitch=pitch)
        kept.append(payload(out, pitch, width, height, bpp))
        check_small(out, fmt, dec, first, width, height, pitch, f"fused {fmt} image at block {first}")
    outs = [small_out(arena, fmt, w, h) for _, w, h in (far, tail)]
    regions_call(t, [far, tail], outs=[o.view for o, _ in outs], pitches=[p for _, p in outs])
    for (first, width, height), (out, pitch) in zip((far, tail), outs):
        check_small(out, fmt, dec, first, width, height, pitch, f"fused {fmt} region at block {first}")
    if fmt != "bc7":
        return
    # the batch call: the far image of the big buffer and a 64 x 64 buffer of its own; each item as its single call
    small_blocks = np.ascontiguousarray(pat[:256])
    ts = on(dev, oracle.transform_bc7(small_blocks.reshape(-1)))
    big_out, big_pitch = small_out(arena, fmt, far[1], far[2])
    little_out, little_pitch = small_out(arena, fmt, 64, 64)
    image.untransform_decode_bc7_images_batch([(t, [far], {"outs": [big_out.view], "pitches": [big_pitch]}),
                                               (ts, [(0, 64, 64)], {"outs": [little_out.view], "pitches": [little_pitch]})])
    assert np.array_equal(payload(big_out, big_pitch, far[1], far[2], bpp), kept[0])
    alone, alone_pitch = small_out(arena, fmt, 64, 64)
    image.untransform_decode_bc7_image(ts, 64, 64, out=alone.view, pitch=alone_pitch)
    assert np.array_equal(payload(little_out, little_pitch, 64, 64, bpp), payload(alone, alone_pitch, 64, 64, bpp))
    check_small(big_out, fmt, dec, far[0], far[1], far[2], big_pitch, "BC7 batch, the far image")
    check_small(little_out, fmt, dec, 0, 64, 64, little_pitch, "BC7 batch, the small buffer")


TILE_CASES = [("bc1", (1, False, True)), ("bc1", (2, False, True)), ("bc3", (1, True, True)), ("bc4", (0, False, False))]


def forward_settings(pkg, fmt, settings):
    mode, sa, sc = settings
    if fmt == "bc1":
        return pkg.Bc1TransformSettings(pkg.YCoCgVariant(mode), sc)
    if fmt == "bc3":
        return pkg.Bc3TransformSettings(pkg.YCoCgVariant(mode), sa, sc)
    return pkg.Bc4TransformSettings(sa)


def fused_tile_call(fmt, settings):
    from dxt_lossless_transform_amd import image

    mode, sa, sc = settings
    if fmt in ("bc4", "bc5"):
        return functools.partial(image.untransform_decode_channel_image, fmt, split_endpoints=sa)
    return functools.partial(image.untransform_decode_image, fmt, decorrelation_mode=mode, split_alpha_endpoints=sa, split_colour_endpoints=sc)


@pytest.mark.parametrize("fmt,settings", TILE_CASES, ids=[f"{f}-{s[0]}" for f, s in TILE_CASES])
def test_fused_tile_image_calls_beyond_four_gib(pkg, oracle, dev, arena, fmt, settings):
    """a transformed buffer (the library's own forward call on the device, pinned at 8 GiB and more by tests/test_gpu_parity.py) of
    more than 4 GiB that ends in an odd, ragged tail: a 260 x 132 image at a first_block whose byte position is beyond 2^32 and that
    lies across tile boundaries (every multiple of 4096 blocks is one), a 36 x 10 image that ends at the last block, both again in
    one region call, and (BC1, default settings) in one batch call next to a small buffer"""
    from dxt_lossless_transform_amd import image

    bs = W.BLOCK[fmt]
    base = 2**32 // bs
    total = base + 5 * 4096 + 1237
    far, last = (base + 2 * 4096 - 100, 260, 132), (total - 27, 36, 10)
    assert total % 2 == 1 and far[0] * bs > 2**32 and far[0] < base + 2 * 4096 < far[0] + 2145
    pat, dec = decoded(oracle, fmt)
    arena.need(2 * bs * total, f"{fmt} blocks and their transform")
    t = arena.take(bs * total)
    getattr(pkg, f"transform_{fmt}_with_settings")(W.tiled(pat, total, arena), t, forward_settings(pkg, fmt, settings))
    single, bpp, kept = fused_tile_call(fmt, settings), W.BPP[fmt], []
    for first, width, height in (far, last):
        out, pitch = small_out(arena, fmt, width, height)
        single(t, width, height, first_block=first, out=out.view, pitch=pitch)
        kept.append(payload(out, pitch, width, height, bpp))
        check_small(out, fmt, dec, first, width, height, pitch, f"fused {fmt} image at block {first}")
    mode, sa, sc = settings
    outs = [small_out(arena, fmt, w, h) for _, w, h in (far, last)]
    image.untransform_decode_images(fmt, t, [far, last], decorrelation_mode=mode, split_alpha_endpoints=sa, split_colour_endpoints=sc,
                                    outs=[o.view for o, _ in outs], pitches=[p for _, p in outs])
    for (first, width, height), (out, pitch) in zip((far, last), outs):
        check_small(out, fmt, dec, first, width, height, pitch, f"fused {fmt} region at block {first}")
    if (fmt, mode) != ("bc1", 1):
        return
    kw = {"decorrelation_mode": mode, "split_alpha_endpoints": sa, "split_colour_endpoints": sc}
    ts = on(dev, oracle.transform("bc1", np.ascontiguousarray(pat[:256]).reshape(-1), mode, sc, sa))
    big_out, big_pitch = small_out(arena, fmt, far[1], far[2])
    little_out, little_pitch = small_out(arena, fmt, 64, 64)
    image.untransform_decode_images_batch([("bc1", t, [far], {**kw, "outs": [big_out.view], "pitches": [big_pitch]}),
                                           ("bc1", ts, [(0, 64, 64)], {**kw, "outs": [little_out.view], "pitches": [little_pitch]})])
    assert np.array_equal(payload(big_out, big_pitch, far[1], far[2], bpp), kept[0])
    alone, alone_pitch = small_out(arena, fmt, 64, 64)
    single(ts, 64, 64, out=alone.view, pitch=alone_pitch)
    assert np.array_equal(payload(little_out, little_pitch, 64, 64, bpp), payload(alone, alone_pitch, 64, 64, bpp))
    check_small(big_out, fmt, dec, far[0], far[1], far[2], big_pitch, "batch, the far image")
    check_small(little_out, fmt, dec, 0, 64, 64, little_pitch, "batch, the small buffer")


# =========================================================================================================================
# C: pixel offsets beyond 2^32 with a small image
# =========================================================================================================================
FAR_WIDTH = 20
FAR_CASES = [(2**30, 9), (2**32, 2)]   # (pitch less its odd bytes, height): 4 * by * pitch passes 2^32 at block row 1; the pitch itself does
FAR_SETTINGS = {"bc1": (1, False, True), "bc3": (1, True, True), "bc4": (0, False, False), "bc5": (0, True, False)}


def far_pitch(fmt, base):
    return base + (47 if fmt == "bc4" else 48)


def cpu_transform(oracle, fmt, blocks):
    """the CPU statement of the forward transform of a small block array"""
    import bc45_ref
    import bc6h_ref

    flat = np.ascontiguousarray(blocks).reshape(-1)
    if fmt in ("bc1", "bc3"):
        mode, sa, sc = FAR_SETTINGS[fmt]
        return oracle.transform(fmt, flat, mode, sc, sa)
    if fmt in ("bc4", "bc5"):
        return bc45_ref.transform(fmt, flat, FAR_SETTINGS[fmt][1])
    return oracle.transform_bc7(flat) if fmt == "bc7" else bc6h_ref.transform(flat)


def far_calls(fmt):
    """[(name, takes transformed blocks, call(src, width, height, out, pitch))]: every image call of the format"""
    from dxt_lossless_transform_amd import image

    calls = [("plain", False, lambda s, w, h, o, p: plain_image_call(fmt)(s, w, h, out=o, pitch=p)),
             ("plain regions", False, lambda s, w, h, o, p: plain_regions_call(fmt)(s, [(0, w, h)], outs=[o], pitches=[p]))]
    if fmt in ("bc7", "bc6h"):
        single = image.untransform_decode_bc7_image if fmt == "bc7" else image.untransform_decode_bc6h_image
        regions = image.untransform_decode_bc7_images if fmt == "bc7" else image.untransform_decode_bc6h_images
        calls += [("fused", True, lambda s, w, h, o, p: single(s, w, h, out=o, pitch=p)),
                  ("fused regions", True, lambda s, w, h, o, p: regions(s, [(0, w, h)], outs=[o], pitches=[p]))]
        if fmt == "bc7":
            calls.append(("batch", True, lambda s, w, h, o, p: image.untransform_decode_bc7_images_batch(
                [(s, [(0, w, h)], {"outs": [o], "pitches": [p]})])))
        return calls
    mode, sa, sc = FAR_SETTINGS[fmt]
    kw = {"decorrelation_mode": mode, "split_alpha_endpoints": sa, "split_colour_endpoints": sc}
    calls += [("fused", True, lambda s, w, h, o, p: fused_tile_call(fmt, FAR_SETTINGS[fmt])(s, w, h, out=o, pitch=p)),
              ("fused regions", True, lambda s, w, h, o, p: image.untransform_decode_images(fmt, s, [(0, w, h)], outs=[o], pitches=[p], **kw)),
              ("batch", True, lambda s, w, h, o, p: image.untransform_decode_images_batch(
                  [(fmt, s, [(0, w, h)], {**kw, "outs": [o], "pitches": [p]})]))]
    return calls


@pytest.mark.parametrize("base,height", FAR_CASES, ids=["pitch-2^30", "pitch-2^32"])
@pytest.mark.parametrize("fmt", ["bc1", "bc3", "bc4", "bc5", "bc7", "bc6h"])
def test_every_image_sink_with_a_far_pitch(pkg, oracle, dev, arena, fmt, base, height):
    """a 20 x 9 image (5 x 3 blocks, the last block row clipped to one pixel row) whose rows lie 2^30 + 48 bytes apart, and its
    first two rows 2^32 + 48 bytes apart, through the plain and the fused single-image call, the plain and the fused region call and
    the batch call of the format: the pixels against the CPU statement, every other byte of the 8 / 4 GiB still 0xA5"""
    pat, dec = decoded(oracle, fmt)
    pitch, bpp = far_pitch(fmt, base), W.BPP[fmt]
    count = 5 * ((height + 3) // 4)
    blocks = np.ascontiguousarray(pat[:count])
    want = W.small_image_bytes(dec[:count], FAR_WIDTH, height, bpp)
    nbytes = pitch * (height - 1) + bpp * FAR_WIDTH
    assert nbytes > 2**32
    arena.need(nbytes, "the far rows")
    plain, transformed = on(dev, blocks.reshape(-1)), on(dev, cpu_transform(oracle, fmt, blocks))
    out = W.Guarded(arena, nbytes)
    for name, takes_transformed, call in far_calls(fmt):
        call(transformed if takes_transformed else plain, FAR_WIDTH, height, out.view, pitch)
        W.check_small_image(out, pitch, FAR_WIDTH, height, bpp, want, f"{fmt} {name}, pitch {pitch}")   # leaves `out` all 0xA5 again
