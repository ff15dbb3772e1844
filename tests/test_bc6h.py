"""BC6H block transform (docs/BC6H_FORMAT.md, include/dxtlt_bc6h.h), checked without a GPU: the field table against Pillow's
BC6H decoder, records worked out by hand, round trips of the CPU restatement (tests/bc6h_ref.py), the kernels' compile-time
tables and record codec built for the host, the tagged TransformHeader word, the DDS switch, the shard placement and the
Python surface."""
import ctypes as C
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import bc6h_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TF_BC6H = 4
FF_OK, FF_UNKNOWN_FORMAT, FF_CORRUPTED = 0, 4, 5
COUNTS = [0, 1, 1023, 1024, 1025, 3 * 1024 + 7]


def random_fields(rng, k):
    """field values of a class-k block whose pixels decode into [0, 1] (UF16): endpoints below 0.45 of the range"""
    epb = R.WIDTHS[k][0]
    lim = int(0.45 * (1 << epb))
    ep = {}
    for ch in range(3):
        w = int(rng.integers(0, lim))
        ep[(ch, 0)] = w
        for e in range(1, R.n_endpoints(k)):
            dw = R.field_width(k, ch, e)
            if R.TRANSFORMED[k]:
                lo, hi = max(0, w - (1 << (dw - 1))), min(lim - 1, w + (1 << (dw - 1)) - 1)
                ep[(ch, e)] = (int(rng.integers(lo, hi + 1)) - w) & ((1 << dw) - 1)
            else:
                ep[(ch, e)] = int(rng.integers(0, lim))
    return ep


def random_block(rng, k):
    return R.pack_block(k, random_fields(rng, k), int(rng.integers(0, 32)), int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63))


def pillow_rgb8(blocks, dxgi=95):
    """Pillow's decode of a row of blocks, (n, 16, 3) uint8 per block"""
    from PIL import Image

    n = blocks.shape[0]
    data = R.dds_dx10(blocks.tobytes(), 4 * n, 4, dxgi)
    im = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(np.int64)
    return im.reshape(4, n, 4, 3).transpose(1, 0, 2, 3).reshape(n, 16, 3)


def numpy_rgb8(blocks):
    f = np.clip(R.decode(blocks).view(np.float16).astype(np.float32), 0.0, 1.0)
    return (f * 255.0).astype(np.int64)


# ---- the field table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(14))
def test_field_table_against_pillow(k):
    """2000 random blocks per mode decode the same (within 1 per 8-bit channel) with Pillow's BC6H decoder and with the
    numpy decoder built from the field table"""
    pytest.importorskip("PIL", reason="Pillow is not installed: the field-table pin needs its BC6H decoder")
    rng = np.random.default_rng(0xBC6 + k)
    blocks = np.stack([random_block(rng, k) for _ in range(2000)])
    assert (R.block_class(blocks[:, 0]) == k).all()
    diff = np.abs(pillow_rgb8(blocks) - numpy_rgb8(blocks)).max(axis=(1, 2))
    assert (diff <= 1).sum() >= 2000, f"mode class {k}: {(diff > 1).sum()} blocks differ by more than 1"


@pytest.mark.parametrize("k", range(14))
def test_every_endpoint_bit_belongs_to_its_channel(k):
    """flipping one endpoint bit changes, under Pillow's decoder, only the channel the table assigns it to"""
    pytest.importorskip("PIL", reason="Pillow is not installed: the field-table pin needs its BC6H decoder")
    rng = np.random.default_rng(0x6000 + k)
    # a base block whose endpoints sit at a quarter of the range, deltas 0, all indices 0: every pixel shows endpoint w or y
    epb = R.WIDTHS[k][0]
    ep = {(ch, e): (1 << (epb - 2)) if e == 0 or not R.TRANSFORMED[k] else 0 for ch in range(3) for e in range(R.n_endpoints(k))}
    base = R.pack_block(k, ep, int(rng.integers(0, 32)), 0)
    flips, owner = [], []
    for (ch, e), pos in R.FIELDS[k].items():
        for p in pos:
            b = base.copy()
            b[p >> 3] ^= 1 << (p & 7)
            flips.append(b)
            owner.append(ch)
    got = pillow_rgb8(np.stack(flips)) - pillow_rgb8(base[None])[0][None]
    changed = np.abs(got).max(axis=1) > 0                      # (bits, 3)
    for i, ch in enumerate(owner):
        assert not changed[i, [c for c in range(3) if c != ch]].any(), f"class {k}, bit {i}: a foreign channel changed"
    owner = np.array(owner)
    for ch in range(3):   # the high bits of every channel show (the low ones may vanish in 8 bits, x and z under index 0)
        assert changed[owner == ch, ch].any(), f"class {k}: no bit of channel {ch} is visible"


def test_classes_of_byte0():
    b = np.arange(256)
    k = R.block_class(b)
    assert (k[(b & 3) == 0] == 0).all() and (k[(b & 3) == 1] == 1).all()
    for c, code in enumerate(R.MODE_BITS[2:], start=2):
        assert (k[(b & 0x1F) == code] == c).all()
    for code in (19, 23, 27, 31):
        assert (k[(b & 0x1F) == code] == R.RESERVED).all()


# ---- records by hand --------------------------------------------------------------------------------------------------
def bits_of(v, n):
    return [(v >> i) & 1 for i in range(n)]


def test_record_two_region_by_hand():
    """class 0 (2-bit mode 00, 10-bit base, 5-bit deltas): mode | partition | 46 index bits | R w x y z | G ... | B ...
    with R and B of w minus G of w, and the high bytes of the three bases at the top (bytes 13, 14, 15)"""
    ep = {(0, 0): 0x2A5, (1, 0): 0x155, (2, 0): 0x0F0, (0, 1): 3, (0, 2): 17, (0, 3): 30, (1, 1): 5, (1, 2): 9, (1, 3): 21,
          (2, 1): 1, (2, 2): 2, (2, 3): 4}
    idx = 0x2A_BCDE_F012_3456 & ((1 << 46) - 1)
    rec = R.records(R.pack_block(0, ep, 0x13, idx)[None])[0]
    rw, bw = (0x2A5 - 0x155) & 0x3FF, (0x0F0 - 0x155) & 0x3FF
    want = [0, 0] + bits_of(0x13, 5) + bits_of(idx, 46)
    for ch, w0 in ((0, rw), (1, 0x155), (2, bw)):
        want += bits_of(w0 & 3, 2) + bits_of(ep[(ch, 1)], 5) + bits_of(ep[(ch, 2)], 5) + bits_of(ep[(ch, 3)], 5)
    want += bits_of(rw >> 2, 8) + bits_of(0x155 >> 2, 8) + bits_of(bw >> 2, 8)
    assert len(want) == 128
    assert rec.tolist() == np.packbits(np.array(want, dtype=np.uint8), bitorder="little").tolist()


def test_record_one_region_reversed_by_hand():
    """class 13 (mode 01111, 16-bit base stored with bits 15..10 reversed, 4-bit deltas): mode | 63 index bits | R w low 8,
    R x | G w low 8, G x | B w low 8, B x | high bytes of R w, G w, B w"""
    ep = {(0, 0): 0xBEEF, (1, 0): 0x1234, (2, 0): 0x7F01, (0, 1): 0x9, (1, 1): 0x3, (2, 1): 0xC}
    idx = (1 << 63) - 12345
    blk = R.pack_block(13, ep, 0, idx)
    # the reversed field, in the block itself: block bit 5 + 30 + 4 = 39 holds bit 15 of R w, bit 44 its bit 10
    bits = np.unpackbits(blk, bitorder="little")
    assert [int(bits[39 + i]) for i in range(6)] == [(0xBEEF >> (15 - i)) & 1 for i in range(6)]
    rec = R.records(blk[None])[0]
    rw, bw = (0xBEEF - 0x1234) & 0xFFFF, (0x7F01 - 0x1234) & 0xFFFF
    want = bits_of(15, 5) + bits_of(idx, 63)
    for ch, w0 in ((0, rw), (1, 0x1234), (2, bw)):
        want += bits_of(w0 & 0xFF, 8) + bits_of(ep[(ch, 1)], 4)
    want += bits_of(rw >> 8, 8) + bits_of(0x1234 >> 8, 8) + bits_of(bw >> 8, 8)
    assert rec.tolist() == np.packbits(np.array(want, dtype=np.uint8), bitorder="little").tolist()


# ---- round trips ------------------------------------------------------------------------------------------------------
def mixed_blocks(n, seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    k = rng.integers(0, 15, size=n)
    codes = np.array(R.MODE_BITS + (19,), dtype=np.uint8)
    mb = np.where(k <= 1, 3, 0x1F).astype(np.uint8)
    b[:, 0] = (b[:, 0] & ~mb) | codes[k]
    return b


@pytest.mark.parametrize("n", COUNTS)
def test_reference_round_trip(n):
    x = mixed_blocks(n, n).reshape(-1)
    y = R.transform(x)
    assert y.size == x.size
    assert np.array_equal(R.untransform(y), x)
    if n >= 64:
        assert not np.array_equal(y, x)


def test_reserved_blocks_move_unchanged():
    x = mixed_blocks(1024, 7)
    x[:, 0] = (x[:, 0] & 0xE0) | 31
    y = R.transform(x.reshape(-1))
    assert np.array_equal(y[15 * 1024:], x[:, 0])
    assert np.array_equal(y[:8 * 1024].reshape(1024, 8), x[:, 1:9])


def test_streams_of_one_granule():
    """main part: Q8 | Q2 | B0..B4 at sorted positions, F (record byte 0) in block order; tail part: a transform of its own"""
    n = 1024 + 5
    x = mixed_blocks(n, 11)
    y = R.transform(x.reshape(-1))
    g = 1024
    rec = R.records(x[:g])
    order = np.argsort(R.block_class(x[:g, 0]), kind="stable")
    assert np.array_equal(y[:8 * g].reshape(g, 8), rec[order][:, 1:9])
    assert np.array_equal(y[8 * g:10 * g].reshape(g, 2), rec[order][:, 9:11])
    assert np.array_equal(y[14 * g:15 * g], rec[order][:, 15])
    assert np.array_equal(y[15 * g:16 * g], rec[:, 0])
    assert np.array_equal(y[16 * g:], R.transform(x[g:].reshape(-1)))


def test_shipped_layout_shrinks_smooth_hdr():
    """the layout is worth shipping: smaller than the untransformed blocks under zlib-6 on a smooth HDR texture"""
    import sys
    import zlib

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bc6h_synth

    yy, xx = np.mgrid[0:128, 0:128].astype(np.float32)
    img = np.stack([1 + np.sin(xx / 17.0) * np.cos(yy / 23.0), 2 + 0.5 * np.sin((xx + yy) / 31.0), 0.5 + yy / 128.0], axis=2)
    blocks = bc6h_synth.encode((img * 4).astype(np.float32))
    raw = blocks.reshape(-1)
    assert len(set(R.block_class(blocks[:, 0]).tolist())) >= 3
    assert len(zlib.compress(R.transform(raw).tobytes(), 6)) < len(zlib.compress(raw.tobytes(), 6))


# ---- the kernels' tables and record codec -------------------------------------------------------------------------------
def test_header_tables_are_generated():
    text = open(os.path.join(ROOT, "dxt-lossless-transform_amd", "csrc", "bc6h_fields.h")).read()
    a = text.index("// ---- GENERATED by tests/bc6h_ref.py kernel_tables() ----\n")
    b = text.index("// ---- end of GENERATED ----")
    assert text[a:b].split("\n", 1)[1] == R.kernel_tables()


def test_device_header_equals_reference(tmp_path):
    """csrc/bc6h_fields.h (the kernels' record codec) built for the host against bc6h_ref, every class, and the forward
    kernel's record byte 0 from the block alone"""
    so = str(tmp_path / "bc6h_fields_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "bc6h_fields_shim.cpp")])
    l = C.CDLL(so)
    l.shim_bc6h_records.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    l.shim_bc6h_record_byte0.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    n = 30_000
    x = mixed_blocks(n, 5)
    rec = np.empty_like(x)
    l.shim_bc6h_records(x.ctypes.data, rec.ctypes.data, n, 0)
    assert np.array_equal(rec, R.records(x))
    back = np.empty_like(x)
    l.shim_bc6h_records(rec.ctypes.data, back.ctypes.data, n, 1)
    assert np.array_equal(back, x)
    b0 = np.empty(n, dtype=np.uint8)
    l.shim_bc6h_record_byte0(x.ctypes.data, b0.ctypes.data, n)
    assert np.array_equal(b0, rec[:, 0])


# ---- the library, without a device ----------------------------------------------------------------------------------
class DdsBatchItem(C.Structure):
    _fields_ = [("input", C.c_void_p), ("input_len", C.c_size_t), ("output", C.c_void_p), ("output_len", C.c_size_t),
                ("decorrelation_mode", C.c_uint8), ("split_alpha_endpoints", C.c_bool), ("split_colour_endpoints", C.c_bool),
                ("status", C.c_int32)]


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, sz, u32, i32, u64, b = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_uint64, C.c_bool
    l.dxtlt_transform_header_pack_bc6h.argtypes, l.dxtlt_transform_header_pack_bc6h.restype = [], u32
    l.dxtlt_file_formats_enable_bc6h.argtypes, l.dxtlt_file_formats_enable_bc6h.restype = [b], None
    l.dxtlt_dds_transform.argtypes, l.dxtlt_dds_transform.restype = [vp, sz, vp, sz, C.c_uint8, b, b], i32
    l.dxtlt_dds_untransform.argtypes, l.dxtlt_dds_untransform.restype = [vp, sz, vp, sz], i32
    l.dxtlt_dds_transform_batch.argtypes, l.dxtlt_dds_transform_batch.restype = [C.POINTER(DdsBatchItem), sz, b], sz
    l.dxtlt_bc6h_shard_pieces.argtypes = [u64, u64, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    l.dxtlt_bc6h_shard_pieces.restype = i32
    l.dxtlt_transform_bc6h.argtypes, l.dxtlt_transform_bc6h.restype = [vp, vp, sz], i32
    l.dxtlt_bc6h_sort_granule.argtypes, l.dxtlt_bc6h_sort_granule.restype = [], u32
    return l


@pytest.fixture
def bc6h_switch(lib):
    lib.dxtlt_file_formats_enable_bc6h(True)
    yield
    lib.dxtlt_file_formats_enable_bc6h(False)


def test_header_word(lib):
    w = lib.dxtlt_transform_header_pack_bc6h()
    assert w == R.HEADER_WORD
    assert w & 0xF == TF_BC6H and (w >> 16) & 0xFFFF == 0xD175 and (w >> 4) & 0xFFF == 1


def dds_file(width, height, dxgi, payload=b"", mips=1):
    return np.frombuffer(R.dds_dx10(payload, width, height, dxgi, mips), dtype=np.uint8).copy()


def with_word(f, word):
    g = f.copy()
    g[0:4] = np.frombuffer(struct.pack("<I", word), dtype=np.uint8)
    return g


@pytest.mark.parametrize("dxgi", [94, 95, 96])
def test_dds_bc6h_refused_with_the_switch_off(lib, dxgi):
    f = dds_file(8, 8, dxgi, bytes(64))
    out = np.zeros(f.size, dtype=np.uint8)
    assert lib.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, out.size, 1, True, True) == FF_UNKNOWN_FORMAT
    t = with_word(f, lib.dxtlt_transform_header_pack_bc6h())
    assert lib.dxtlt_dds_untransform(t.ctypes.data, t.size, out.ctypes.data, out.size) == FF_UNKNOWN_FORMAT
    items = (DdsBatchItem * 1)()
    items[0].input, items[0].input_len, items[0].output, items[0].output_len = f.ctypes.data, f.size, out.ctypes.data, out.size
    assert lib.dxtlt_dds_transform_batch(items, 1, False) == 1 and items[0].status == FF_UNKNOWN_FORMAT


@pytest.mark.parametrize("dxgi", [94, 95, 96])
def test_dds_bc6h_empty_payload_round_trip_without_a_device(lib, bc6h_switch, dxgi):
    """a 0 x 0 texture has no blocks: the whole handler runs on the host, header word and trailing bytes included"""
    f = dds_file(0, 0, dxgi, b"tail")
    out = np.zeros(f.size, dtype=np.uint8)
    assert lib.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, out.size, 3, True, True) == FF_OK
    assert struct.unpack_from("<I", out.tobytes())[0] == R.HEADER_WORD
    assert out[4:].tobytes() == f[4:].tobytes()
    back = np.zeros(f.size, dtype=np.uint8)
    assert lib.dxtlt_dds_untransform(out.ctypes.data, out.size, back.ctypes.data, back.size) == FF_OK
    assert back.tobytes() == f.tobytes()
    # any other data bits under the BC6H code are refused
    for bad in (TF_BC6H, R.HEADER_WORD ^ (1 << 4), R.HEADER_WORD ^ (1 << 20)):
        t = with_word(out, bad)
        assert lib.dxtlt_dds_untransform(t.ctypes.data, t.size, back.ctypes.data, back.size) == FF_CORRUPTED


def test_length_checked_without_a_device(lib, pkg):
    x = np.zeros(24, dtype=np.uint8)
    assert lib.dxtlt_transform_bc6h(x.ctypes.data, x.ctypes.data, 24) != 0
    assert lib.dxtlt_transform_bc6h(x.ctypes.data, x.ctypes.data, 0) == 0
    assert lib.dxtlt_bc6h_sort_granule() == 1024


@pytest.mark.parametrize("total,first,num", [(5000, 0, 5000), (5000, 1024, 2048), (5000, 3072, 1928), (4096, 2048, 2048),
                                             (700, 0, 700), (3 * 1024 + 7, 2048, 1031)])
def test_shard_pieces(lib, total, first, num):
    g, lo, nb = (C.c_uint64 * 9)(), (C.c_uint64 * 9)(), (C.c_uint64 * 9)()
    assert lib.dxtlt_bc6h_shard_pieces(total, first, num, g, lo, nb) == 0
    assert (list(g), list(lo), list(nb)) == R.shard_pieces(total, first, num)
    # the pieces of a stand-alone shard transform land where the whole buffer's transform has them
    x = mixed_blocks(total, total).reshape(-1)
    whole = R.transform(x)
    part = R.transform(x[16 * first:16 * (first + num)])
    for p in range(9):
        assert np.array_equal(whole[g[p]:g[p] + nb[p]], part[lo[p]:lo[p] + nb[p]])


def test_shard_pieces_refuse_unaligned(lib):
    g, lo, nb = (C.c_uint64 * 9)(), (C.c_uint64 * 9)(), (C.c_uint64 * 9)()
    assert lib.dxtlt_bc6h_shard_pieces(5000, 100, 1024, g, lo, nb) != 0
    assert lib.dxtlt_bc6h_shard_pieces(5000, 0, 1000, g, lo, nb) != 0


def test_python_surface(pkg):
    from dxt_lossless_transform_amd import batch, bc6h

    for name in ("transform_bc6h", "untransform_bc6h", "sort_granule", "transform_bc6h_range", "transform_bc6h_sharded",
                 "shard_pieces"):
        assert callable(getattr(bc6h, name)), name
    assert bc6h.sort_granule() == 1024
    assert bc6h.shard_pieces(5000, 0, 5000) == tuple(R.shard_pieces(5000, 0, 5000)) or \
        list(bc6h.shard_pieces(5000, 0, 5000)) == list(R.shard_pieces(5000, 0, 5000))
    assert batch._item_fields("bc6h", None) == (6, 16, 0, False, False)
