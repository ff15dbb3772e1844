"""The BC7 decoder as a plain numpy statement (docs/IMAGE_DECODE.md, "BC7"), written from the definition -- the Direct3D 11
decoder -- one field at a time, with the tables as the format's documents print them (a digit per pixel, an anchor per
partition).  It shares nothing with csrc/bc7_decode.h, which packs the tables and never walks a block pixel by pixel.

decode_blocks(blocks) -> (N, 64) uint8: sixteen r, g, b, a pixels per block, pixel 4 r + c at (c, r).  The reserved encoding
(byte 0 == 0) gives 64 zero bytes.  Also here: the block generators of the BC7 tests and the image assembly."""
import numpy as np

# subset of every pixel, per partition (row-major, pixel 0 first)
PARTITION2 = """
    0011001100110011 0001000100010001 0111011101110111 0001001100110111
    0000000100010011 0011011101111111 0001001101111111 0000000100110111
    0000000000010011 0011011111111111 0000000101111111 0000000000010111
    0001011111111111 0000000011111111 0000111111111111 0000000000001111
    0000100011101111 0111000100000000 0000000010001110 0111001100010000
    0011000100000000 0000100011001110 0000000010001100 0111001100110001
    0011000100010000 0000100010001100 0110011001100110 0011011001101100
    0001011111101000 0000111111110000 0111000110001110 0011100110011100
    0101010101010101 0000111100001111 0101101001011010 0011001111001100
    0011110000111100 0101010110101010 0110100101101001 0101101010100101
    0111001111001110 0001001111001000 0011001001001100 0011101111011100
    0110100110010110 0011110011000011 0110011010011001 0000011001100000
    0100111001000000 0010011100100000 0000001001110010 0000010011100100
    0110110010010011 0011011011001001 0110001110011100 0011100111000110
    0110110011001001 0110001100111001 0111111010000001 0001100011100111
    0000111100110011 0011001111110000 0010001011101110 0100010001110111
""".split()
PARTITION3 = """
    0011001102212222 0001001122112221 0000200122112211 0222002200110111
    0000000011221122 0011001100220022 0022002211111111 0011001122112211
    0000000011112222 0000111111112222 0000111122222222 0012001200120012
    0112011201120112 0122012201220122 0011011211221222 0011200122002220
    0001001101121122 0111001120012200 0000112211221122 0022002200221111
    0111011102220222 0001000122212221 0000001101220122 0000110022102210
    0122012200110000 0012001211222222 0110122112210110 0000011012211221
    0022110211020022 0110011020022222 0011012201220011 0000200022112221
    0000000211221222 0222002200120011 0011001200220222 0120012001200120
    0000111122220000 0120120120120120 0120201212010120 0011220011220011
    0011112222000011 0101010122222222 0000000021212121 0022112200221122
    0022001100220011 0220122102201221 0101222222220101 0000212121212121
    0101010101012222 0222011102220111 0002111200021112 0000211221122112
    0222011101110222 0002111211120002 0110011001102222 0000000021122112
    0110011022222222 0022001100110022 0022112211220022 0000000000002112
    0002000100020001 0222122202221222 0101222222222222 0111201122012220
""".split()
# anchor pixel of the second subset (two subsets), of the second and of the third subset (three subsets)
ANCHOR2 = [
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15,  2,  8,  2,  2,  8,  8, 15,  2,  8,  2,  2,  8,  8,  2,  2,
    15, 15,  6,  8,  2,  8, 15, 15,  2,  8,  2,  2,  2, 15, 15,  6,
     6,  2,  6,  8, 15, 15,  2,  2, 15, 15, 15, 15, 15,  2,  2, 15,
]
ANCHOR3_SECOND = [
     3,  3, 15, 15,  8,  3, 15, 15,  8,  8,  6,  6,  6,  5,  3,  3,
     3,  3,  8, 15,  3,  3,  6, 10,  5,  8,  8,  6,  8,  5, 15, 15,
     8, 15,  3,  5,  6, 10,  8, 15, 15,  3, 15,  5, 15, 15, 15, 15,
     3, 15,  5,  5,  5,  8,  5, 10,  5, 10,  8, 13, 15, 12,  3,  3,
]
ANCHOR3_THIRD = [
    15,  8,  8,  3, 15, 15,  3,  8, 15, 15, 15, 15, 15, 15, 15,  8,
    15,  8, 15,  3, 15,  8, 15,  8,  3, 15,  6, 10, 15, 15, 10,  8,
    15,  3, 15, 10, 10,  8,  9, 10,  6, 15,  8, 15,  3,  6,  6,  8,
    15,  3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,  3, 15, 15,  8,
]
WEIGHTS = {2: [0, 21, 43, 64], 3: [0, 9, 18, 27, 37, 46, 55, 64], 4: [0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64]}
# per mode: subsets, partition bits, rotation bits, index selector bits, colour bits, alpha bits, p-bits per endpoint, p-bits
# per subset, index bits, second index bits
MODES = [
    (3, 4, 0, 0, 4, 0, 1, 0, 3, 0),
    (2, 6, 0, 0, 6, 0, 0, 1, 3, 0),
    (3, 6, 0, 0, 5, 0, 0, 0, 2, 0),
    (2, 6, 0, 0, 7, 0, 1, 0, 2, 0),
    (1, 0, 2, 1, 5, 6, 0, 0, 2, 3),
    (1, 0, 2, 0, 7, 8, 0, 0, 2, 2),
    (1, 0, 0, 0, 7, 7, 1, 0, 4, 0),
    (2, 6, 0, 0, 5, 5, 1, 0, 2, 0),
]
_P2 = np.array([[int(c) for c in s] for s in PARTITION2], dtype=np.int64)
_P3 = np.array([[int(c) for c in s] for s in PARTITION3], dtype=np.int64)
_A2, _A3S, _A3T = (np.array(a, dtype=np.int64) for a in (ANCHOR2, ANCHOR3_SECOND, ANCHOR3_THIRD))
U64 = np.uint64


def _bits(lo, hi, pos, n):
    """bits [pos, pos + n) of the 128-bit little-endian numbers (lo, hi); pos and n: ints or per-block arrays, n <= 32"""
    pos = np.broadcast_to(np.asarray(pos, dtype=np.int64), lo.shape)
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), lo.shape)
    low_part = np.where(pos < 64, lo >> np.minimum(pos, 63).astype(U64), U64(0))
    carry = np.where((pos > 0) & (pos < 64), hi << ((64 - np.clip(pos, 1, 63)).astype(U64)), U64(0))
    high_part = np.where(pos >= 64, hi >> np.clip(pos - 64, 0, 63).astype(U64), U64(0))
    return ((low_part | carry | high_part) & ((U64(1) << n.astype(U64)) - U64(1))).astype(np.int64)


def block_modes(blocks):
    """mode 0..7 of every block, 8 for the reserved encoding"""
    b0 = np.asarray(blocks, dtype=np.uint8).reshape(-1, 16)[:, 0].astype(np.int64) | 0x100
    return np.log2(b0 & -b0).astype(np.int64)


def _decode_mode(m, lo, hi):
    ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[m]
    n = lo.shape[0]
    pos = m + 1
    partition = _bits(lo, hi, pos, pb); pos += pb
    rotation = _bits(lo, hi, pos, rb); pos += rb
    selector = _bits(lo, hi, pos, isb); pos += isb
    ends = np.zeros((n, 2 * ns, 4), dtype=np.int64)   # endpoint, channel
    for ch in range(3):
        for e in range(2 * ns):
            ends[:, e, ch] = _bits(lo, hi, pos, cb); pos += cb
    for e in range(2 * ns if ab else 0):
        ends[:, e, 3] = _bits(lo, hi, pos, ab); pos += ab
    widths = [cb, cb, cb, ab]
    if epb or spb:
        for e in range(2 * ns):
            p = _bits(lo, hi, pos + (e if epb else e // 2), 1)
            ends[:, e, :] = (ends[:, e, :] << 1) | p[:, None]
        pos += 2 * ns if epb else ns
        widths = [w + 1 if w else 0 for w in widths]
    for ch, w in enumerate(widths):
        if w:
            ends[:, :, ch] = ((ends[:, :, ch] << (8 - w)) | (ends[:, :, ch] >> (2 * w - 8))) & 255
        else:
            ends[:, :, ch] = 255
    if ns == 1:
        subset = np.zeros((n, 16), dtype=np.int64)
        anchors = np.zeros((n, 1), dtype=np.int64)
    elif ns == 2:
        subset = _P2[partition]
        anchors = np.stack([np.zeros(n, np.int64), _A2[partition]], axis=1)
    else:
        subset = _P3[partition]
        anchors = np.stack([np.zeros(n, np.int64), _A3S[partition], _A3T[partition]], axis=1)

    def index_set(pos, width, anchors):
        out = np.zeros((n, 16), dtype=np.int64)
        at = np.full(n, pos, dtype=np.int64)
        for i in range(16):
            w = width - (anchors == i).any(axis=1).astype(np.int64)
            out[:, i] = _bits(lo, hi, at, w)
            at = at + w
        return out, at

    first, at = index_set(pos, ib, anchors)
    colour_w = np.array(WEIGHTS[ib], dtype=np.int64)[first]
    alpha_w = colour_w
    if ib2:
        second, at = index_set(at[0], ib2, np.zeros((n, 1), dtype=np.int64))
        second_w = np.array(WEIGHTS[ib2], dtype=np.int64)[second]
        swap = (selector == 1)[:, None]
        colour_w, alpha_w = np.where(swap, second_w, colour_w), np.where(swap, colour_w, second_w)
    assert (at == 128).all()
    rows = np.arange(n)[:, None]
    e0, e1 = ends[rows, 2 * subset], ends[rows, 2 * subset + 1]   # (n, 16, 4)
    w = np.stack([colour_w, colour_w, colour_w, alpha_w], axis=2)
    px = ((64 - w) * e0 + w * e1 + 32) >> 6
    for r in (1, 2, 3):
        sel = rotation == r
        px[sel, :, 3], px[sel, :, r - 1] = px[sel, :, r - 1].copy(), px[sel, :, 3].copy()
    return px.astype(np.uint8).reshape(n, 64)


def decode_blocks(blocks):
    blocks = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint8).reshape(-1, 16))
    halves = blocks.view("<u8")
    lo, hi = halves[:, 0].copy(), halves[:, 1].copy()
    modes = block_modes(blocks)
    out = np.zeros((blocks.shape[0], 64), dtype=np.uint8)
    for m in range(8):
        sel = np.nonzero(modes == m)[0]
        if sel.size:
            out[sel] = _decode_mode(m, lo[sel], hi[sel])
    return out


def image_of(pixels, width, height):
    """(height, width, 4) image of the row-major blocks' (N, 64) pixels; blocks beyond the edge are clipped"""
    bw, bh = (width + 3) // 4, (height + 3) // 4
    px = np.asarray(pixels, dtype=np.uint8)[:bw * bh].reshape(bh, bw, 4, 4, 4)
    return np.ascontiguousarray(px.transpose(0, 2, 1, 3, 4).reshape(4 * bh, 4 * bw, 4)[:height, :width])


# ---- block generators ------------------------------------------------------------------------------------------------------
def with_mode(blocks, modes):
    """the (N, 16) blocks with the mode marker of `modes` (0..7; 8 = reserved) in byte 0, the other bits as they are"""
    blocks = np.array(blocks, dtype=np.uint8).reshape(-1, 16)
    modes = np.asarray(modes, dtype=np.int64)
    keep = (0xFF << (modes + 1)) & 0xFF
    blocks[:, 0] = (blocks[:, 0] & keep) | np.where(modes < 8, 1 << np.minimum(modes, 7), 0)
    return blocks


def mode_balanced_blocks(n, seed):
    """random blocks whose mode is drawn uniformly from 0..7 (plain random bytes are half mode 0 and 1 / 256 mode 7)"""
    rng = np.random.default_rng(seed)
    return with_mode(rng.integers(0, 256, (n, 16), dtype=np.uint8), rng.integers(0, 8, n))


def single_mode_blocks(n, mode, seed):
    rng = np.random.default_rng(seed)
    return with_mode(rng.integers(0, 256, (n, 16), dtype=np.uint8), np.full(n, mode))


def wave_uniform_blocks(n, seed):
    """every run of 64 blocks of one mode, each mode in turn"""
    rng = np.random.default_rng(seed)
    return with_mode(rng.integers(0, 256, (n, 16), dtype=np.uint8), (np.arange(n) // 64) % 8)


def interleaved_class_blocks(n, seed):
    """all nine classes, the reserved encoding included, side by side in every wave"""
    rng = np.random.default_rng(seed)
    return with_mode(rng.integers(0, 256, (n, 16), dtype=np.uint8), np.arange(n) % 9)
