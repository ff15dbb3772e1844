"""BC4 / BC5 block transforms (docs/BC45_FORMAT.md, include/dxtlt_bc45.h), checked without a GPU: the CPU restatement against
hand-built vectors, the Python stream table, the tagged TransformHeader words, the DDS switch (refusal with it off, item-by-item
validation with it on) and the host planning of the single-buffer and batch launches for formats 4 and 5."""
import ctypes as C
import struct

import numpy as np
import pytest

import bc45_ref

TF_BC4, TF_BC5 = 8, 9
FF_OK, FF_INPUT_TOO_SHORT, FF_UNKNOWN_FORMAT, FF_CORRUPTED = 0, 3, 4, 5


class Launch(C.Structure):
    _fields_ = [("kind", C.c_int32), ("threads", C.c_int32), ("workgroups", C.c_uint32), ("full_tiles", C.c_uint32),
                ("range_blocks", C.c_uint64), ("aos_offset", C.c_uint64), ("shift", C.c_uint8 * 6), ("halo_vecs", C.c_uint8),
                ("natural", C.c_uint8), ("gbase", C.c_uint64 * 6)]


class Entry(C.Structure):
    _fields_ = [("first_wg", C.c_uint32), ("end_wg", C.c_uint32), ("full_tiles", C.c_uint32), ("form", C.c_uint8),
                ("halo_vecs", C.c_uint8), ("shift", C.c_uint8 * 6), ("gbase", C.c_uint64 * 6)]


class DdsBatchItem(C.Structure):
    _fields_ = [("input", C.c_void_p), ("input_len", C.c_size_t), ("output", C.c_void_p), ("output_len", C.c_size_t),
                ("decorrelation_mode", C.c_uint8), ("split_alpha_endpoints", C.c_bool), ("split_colour_endpoints", C.c_bool),
                ("status", C.c_int32)]


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, sz, u32, i32, u64, b = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_uint64, C.c_bool
    l.dxtlt_transform_header_pack_bc45.argtypes, l.dxtlt_transform_header_pack_bc45.restype = [i32, b], u32
    l.dxtlt_transform_header_unpack_reserved_format.argtypes = [u32, C.POINTER(i32), C.POINTER(b)]
    l.dxtlt_transform_header_unpack_reserved_format.restype = i32
    l.dxtlt_transform_header_pack_reserved_format.argtypes, l.dxtlt_transform_header_pack_reserved_format.restype = [i32, b], u32
    l.dxtlt_file_formats_enable_bc45.argtypes, l.dxtlt_file_formats_enable_bc45.restype = [b], None
    l.dxtlt_dds_transform.argtypes, l.dxtlt_dds_transform.restype = [vp, sz, vp, sz, C.c_uint8, b, b], i32
    l.dxtlt_dds_untransform.argtypes, l.dxtlt_dds_untransform.restype = [vp, sz, vp, sz], i32
    l.dxtlt_dds_transform_batch.argtypes, l.dxtlt_dds_transform_batch.restype = [C.POINTER(DdsBatchItem), sz, b], sz
    l.dxtlt_debug_plan_transform.argtypes = [i32, i32, i32, i32, i32, u64, u64, u64, u64, u64, C.POINTER(Launch), i32]
    l.dxtlt_debug_plan_transform.restype = i32
    l.dxtlt_debug_plan_batch.argtypes = [i32, i32, i32, i32, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), sz,
                                         C.POINTER(Entry), C.POINTER(C.c_uint8), sz, C.POINTER(u32)]
    l.dxtlt_debug_plan_batch.restype = u32
    for n in ("bc4", "bc5"):
        for d in ("transform", "untransform"):
            f = getattr(l, f"dxtlt_{d}_{n}_with_settings")
            f.argtypes, f.restype = [vp, vp, sz, b], i32
    return l


@pytest.fixture
def bc45_switch(lib):
    """the process-wide DDS switch, on for the test and off again behind it"""
    lib.dxtlt_file_formats_enable_bc45(True)
    yield
    lib.dxtlt_file_formats_enable_bc45(False)


# ---- the layout ------------------------------------------------------------------------------------------------
def blocks_of(fmt, n):
    """block i, byte j = 16 i + j + 1 (every byte distinct for n <= 15)"""
    B = bc45_ref.BLOCK[fmt]
    return [[(16 * i + j + 1) & 0xFF for j in range(B)] for i in range(n)]


def by_hand(fmt, blocks, split):
    """the table of docs/BC45_FORMAT.md spelled out field by field"""
    out = []
    for h in range(2 if fmt == "bc5" else 1):
        o = 8 * h
        if split:
            out += [b[o + 0] for b in blocks]
            out += [b[o + 1] for b in blocks]
        else:
            for b in blocks:
                out += [b[o + 0], b[o + 1]]
        for b in blocks:
            out += b[o + 2:o + 8]
    return out


def test_reference_against_literal_vectors():
    two = np.array(sum(blocks_of("bc4", 2), []), dtype=np.uint8)
    # BC4, 2 blocks: a0 a1 of both, then both index records
    assert bc45_ref.transform("bc4", two, False).tolist() == [1, 2, 17, 18, 3, 4, 5, 6, 7, 8, 19, 20, 21, 22, 23, 24]
    assert bc45_ref.transform("bc4", two, True).tolist() == [1, 17, 2, 18, 3, 4, 5, 6, 7, 8, 19, 20, 21, 22, 23, 24]
    two5 = np.array(sum(blocks_of("bc5", 2), []), dtype=np.uint8)
    assert bc45_ref.transform("bc5", two5, False).tolist() == [
        1, 2, 17, 18, 3, 4, 5, 6, 7, 8, 19, 20, 21, 22, 23, 24,
        9, 10, 25, 26, 11, 12, 13, 14, 15, 16, 27, 28, 29, 30, 31, 32]
    assert bc45_ref.transform("bc5", two5, True).tolist() == [
        1, 17, 2, 18, 3, 4, 5, 6, 7, 8, 19, 20, 21, 22, 23, 24,
        9, 25, 10, 26, 11, 12, 13, 14, 15, 16, 27, 28, 29, 30, 31, 32]


@pytest.mark.parametrize("fmt", ["bc4", "bc5"])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_reference_against_hand_built_vectors(fmt, split, n):
    blocks = blocks_of(fmt, n)
    aos = np.array(sum(blocks, []), dtype=np.uint8)
    want = by_hand(fmt, blocks, split)
    got = bc45_ref.transform(fmt, aos, split)
    assert got.tolist() == want
    assert got.size == aos.size
    assert bc45_ref.untransform(fmt, got, split).tolist() == aos.tolist()
    if n == 1:
        assert got.tolist() == aos.tolist()           # one block: every stream holds one record, in block order


def test_stream_table(pkg):
    assert pkg.stream_table("bc4", pkg.Bc4TransformSettings()) == [(0, 2), (2, 6)]
    assert pkg.stream_table("bc4", pkg.Bc4TransformSettings(True)) == [(0, 1), (1, 1), (2, 6)]
    assert pkg.stream_table("bc5", pkg.Bc5TransformSettings()) == [(0, 2), (2, 6), (8, 2), (10, 6)]
    assert pkg.stream_table("bc5", pkg.Bc5TransformSettings(True)) == [(0, 1), (1, 1), (2, 6), (8, 1), (9, 1), (10, 6)]
    for fmt, S in (("bc4", pkg.Bc4TransformSettings), ("bc5", pkg.Bc5TransformSettings)):
        assert [s.split_endpoints for s in S.all_combinations()] == [False, True]
        assert S() == S(False)
        for s in S.all_combinations():
            assert pkg.stream_table(fmt, s) == bc45_ref.streams(fmt, s.split_endpoints)
    assert pkg.BLOCK_BYTES["bc4"] == 8 and pkg.BLOCK_BYTES["bc5"] == 16
    for name in ("Bc4TransformSettings", "Bc5TransformSettings", "transform_bc4_with_settings", "untransform_bc4_with_settings",
                 "transform_bc5_with_settings", "untransform_bc5_with_settings"):
        assert name in pkg.__all__


def test_host_calls_validate_without_a_device(lib):
    p = (C.c_uint8 * 64)()
    assert lib.dxtlt_transform_bc4_with_settings(p, p, 12, False) == 1          # not a multiple of 8
    assert lib.dxtlt_untransform_bc5_with_settings(p, p, 24, True) == 1         # not a multiple of 16
    assert lib.dxtlt_transform_bc5_with_settings(None, p, 16, False) == 2       # NULL with len > 0
    assert lib.dxtlt_transform_bc4_with_settings(p, p, 0, True) == 0            # zero blocks: nothing to do, no device needed


# ---- TransformHeader ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [TF_BC4, TF_BC5])
@pytest.mark.parametrize("split", [False, True])
def test_tagged_header_words(lib, code, split):
    word = lib.dxtlt_transform_header_pack_bc45(code, split)
    data = word >> 4
    assert word & 0xF == code
    assert data & 3 == 0                       # upstream's placeholder version
    assert (data >> 2) & 1 == int(split)       # split_endpoints
    assert (data >> 3) & 0x1FF == 1            # this build's layout version
    assert data >> 12 == 0xD175                # vendor tag
    f, flag = C.c_int32(-1), C.c_bool(False)
    # upstream's placeholder unpack refuses the word (reserved bits set), and so does this library's replay of it
    assert lib.dxtlt_transform_header_unpack_reserved_format(word, C.byref(f), C.byref(flag)) == FF_CORRUPTED
    assert word != lib.dxtlt_transform_header_pack_reserved_format(code, split)


def test_tagged_header_words_only_for_bc4_bc5(lib):
    for code in (0, 1, 2, 3, 4, 5, 6, 7, 10, 15):
        assert lib.dxtlt_transform_header_pack_bc45(code, True) == 0
    assert lib.dxtlt_transform_header_pack_bc45(TF_BC4, False) != lib.dxtlt_transform_header_pack_bc45(TF_BC4, True)


# ---- DDS ---------------------------------------------------------------------------------------------------------
def dds(fourcc: bytes, width: int, height: int, payload: bytes = b"", mips: int = 0, dxgi: int = None) -> np.ndarray:
    h = bytearray(128)
    h[0:4] = b"DDS "
    struct.pack_into("<I", h, 4, 124)
    struct.pack_into("<III", h, 8, 0x1 | 0x2 | 0x4 | 0x1000 | (0x20000 if mips else 0), height, width)
    struct.pack_into("<I", h, 0x1C, mips)
    struct.pack_into("<II", h, 0x4C, 32, 0x4)
    h[0x54:0x58] = fourcc
    if dxgi is not None:
        h += struct.pack("<IIIII", dxgi, 3, 0, 1, 0)
    return np.frombuffer(bytes(h) + payload, dtype=np.uint8).copy()


def items_of(files, inverse_outs=None):
    items = (DdsBatchItem * len(files))()
    outs = [np.zeros(max(1, f.size), dtype=np.uint8) for f in files]
    for it, f, o in zip(items, files, outs):
        it.input, it.input_len, it.output, it.output_len = f.ctypes.data, f.size, o.ctypes.data, o.size
        it.decorrelation_mode, it.split_alpha_endpoints, it.split_colour_endpoints, it.status = 1, True, True, -1
    return items, outs


@pytest.mark.parametrize("fourcc,dxgi", [(b"ATI1", None), (b"BC4U", None), (b"BC4S", None), (b"ATI2", None), (b"BC5U", None),
                                         (b"BC5S", None), (b"DX10", 80), (b"DX10", 81), (b"DX10", 83), (b"DX10", 84)])
def test_dds_bc45_refused_with_the_switch_off(lib, fourcc, dxgi):
    f = dds(fourcc, 8, 8, bytes(64), dxgi=dxgi)
    out = np.zeros(f.size, dtype=np.uint8)
    assert lib.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, out.size, 1, True, True) == FF_UNKNOWN_FORMAT
    t = f.copy()
    t[0:4] = np.frombuffer(struct.pack("<I", lib.dxtlt_transform_header_pack_bc45(TF_BC4, False)), dtype=np.uint8)
    assert lib.dxtlt_dds_untransform(t.ctypes.data, t.size, out.ctypes.data, out.size) == FF_UNKNOWN_FORMAT
    items, _ = items_of([f])
    assert lib.dxtlt_dds_transform_batch(items, 1, False) == 1 and items[0].status == FF_UNKNOWN_FORMAT
    items, _ = items_of([t])
    assert lib.dxtlt_dds_transform_batch(items, 1, True) == 1 and items[0].status == FF_UNKNOWN_FORMAT


@pytest.mark.parametrize("fourcc,code", [(b"ATI1", TF_BC4), (b"BC5U", TF_BC5)])
@pytest.mark.parametrize("split", [False, True])
def test_dds_bc45_empty_payload_round_trip_without_a_device(lib, bc45_switch, fourcc, code, split):
    """A 0 x 0 texture has no blocks: the whole handler runs on the host, header word and trailing bytes included."""
    f = dds(fourcc, 0, 0, b"tail")
    out = np.zeros(f.size, dtype=np.uint8)
    assert lib.dxtlt_dds_transform(f.ctypes.data, f.size, out.ctypes.data, out.size, 3, split, True) == FF_OK
    assert struct.unpack_from("<I", out.tobytes())[0] == lib.dxtlt_transform_header_pack_bc45(code, split)
    assert out[4:].tobytes() == f[4:].tobytes()
    back = np.zeros(f.size, dtype=np.uint8)
    assert lib.dxtlt_dds_untransform(out.ctypes.data, out.size, back.ctypes.data, back.size) == FF_OK
    assert back.tobytes() == f.tobytes()


def test_dds_batch_validates_bc45_item_by_item_without_a_device(lib, bc45_switch):
    """With the switch on every BC4 / BC5 item gets the single call's status; none of these reaches the device."""
    tagged4 = lib.dxtlt_transform_header_pack_bc45(TF_BC4, True)
    empty4, empty5 = dds(b"ATI1", 0, 0), dds(b"DX10", 0, 0, dxgi=83)
    short5 = dds(b"ATI2", 8, 8, bytes(40))                                      # 4 blocks of 16 bytes stated, 40 bytes follow
    files = [empty4, empty5, short5]
    items, outs = items_of(files)
    assert lib.dxtlt_dds_transform_batch(items, len(files), False) == 1
    assert [it.status for it in items] == [FF_OK, FF_OK, FF_INPUT_TOO_SHORT]
    assert struct.unpack_from("<I", outs[0].tobytes())[0] == tagged4                  # split_alpha_endpoints = True carries the split
    assert struct.unpack_from("<I", outs[1].tobytes())[0] == lib.dxtlt_transform_header_pack_bc45(TF_BC5, True)

    def with_word(f, word):
        g = f.copy()
        g[0:4] = np.frombuffer(struct.pack("<I", word), dtype=np.uint8)
        return g

    upstream_style = lib.dxtlt_transform_header_pack_reserved_format(TF_BC4, True)    # version 0 | flag, no tag
    inv = [with_word(empty4, tagged4), with_word(empty4, upstream_style), with_word(empty4, tagged4 ^ (1 << 20)),
           with_word(empty5, lib.dxtlt_transform_header_pack_bc45(TF_BC5, False)), with_word(empty5, (tagged4 & ~0xF | TF_BC5) ^ (1 << 7))]   # layout version 0
    items, outs = items_of(inv)
    assert lib.dxtlt_dds_transform_batch(items, len(inv), True) == 3
    assert [it.status for it in items] == [FF_OK, FF_CORRUPTED, FF_CORRUPTED, FF_OK, FF_CORRUPTED]
    assert outs[0].tobytes() == empty4.tobytes() and outs[3].tobytes() == empty5.tobytes()
    # the single call agrees
    out = np.zeros(empty4.size, dtype=np.uint8)
    assert lib.dxtlt_dds_untransform(inv[1].ctypes.data, inv[1].size, out.ctypes.data, out.size) == FF_CORRUPTED


# ---- host planning of the launches ---------------------------------------------------------------------------------
def plan(lib, fmt, inverse, split, src, dst, total, first, num, variant=1, split_colour=1):
    out = (Launch * 16)()
    n = lib.dxtlt_debug_plan_transform(fmt, int(inverse), variant, int(split), split_colour, src, dst, total, first, num, out, 16)
    return n, list(out)[:max(0, min(n, 16))]


@pytest.mark.parametrize("fmt", [4, 5])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_plan_transform_aligned(lib, fmt, split, inverse):
    lanes = 128 if fmt == 4 else 256                       # BC1's / BC3's aligned tile widths
    T = lanes * 16 // bc45_ref.BLOCK[{4: "bc4", 5: "bc5"}[fmt]]
    N = 4096 * T
    n, ls = plan(lib, fmt, inverse, split, 1 << 40, 1 << 41, N, 0, N)
    assert n == 1
    assert (ls[0].kind, ls[0].threads, ls[0].workgroups, ls[0].full_tiles) == (0, lanes, 4096, 4096)
    # decorrelation mode and colour split are ignored for these formats
    assert plan(lib, fmt, inverse, split, 1 << 40, 1 << 41, N, 0, N, variant=3, split_colour=0)[0] == 1


@pytest.mark.parametrize("fmt", [4, 5])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_plan_transform_odd_count(lib, fmt, split, inverse):
    name = {4: "bc4", 5: "bc5"}[fmt]
    N = 4 * 4096 + 1
    soa = 1 << 41
    n, ls = plan(lib, fmt, inverse, split, soa if inverse else 1 << 40, 1 << 40 if inverse else soa, N, 0, N)
    assert n == 1
    l = ls[0]
    T = 256 * 16 // bc45_ref.BLOCK[name]                    # halo / shifted / edge tiles: 256 lanes
    assert (l.kind, l.threads) == ((2 if inverse else 1), 256)
    assert l.full_tiles == N // T and l.workgroups == l.full_tiles + 1      # whole tiles, then the edge tile
    assert l.range_blocks == N
    S = bc45_ref.streams(name, split)
    mask = 15 if inverse else 63
    assert list(l.shift)[:len(S)] == [(soa + off * N) & mask for off, w in S]
    assert list(l.shift)[len(S):] == [0] * (6 - len(S))
    assert list(l.gbase)[:len(S)] == [off * N - ((soa + off * N) & mask) for off, w in S]


def test_plan_transform_refuses_other_formats(lib):
    for fmt in (0, 6, 7, 8, 9, 15):
        assert plan(lib, fmt, False, False, 1 << 40, 1 << 41, 1024, 0, 1024)[0] == -1


@pytest.mark.parametrize("fmt", [4, 5])
@pytest.mark.parametrize("inverse", [False, True])
def test_plan_batch(lib, fmt, inverse):
    name = {4: "bc4", 5: "bc5"}[fmt]
    T = 256 * 16 // bc45_ref.BLOCK[name]                    # batch tiles: 256 lanes
    blocks = [64 * T, 3 * T + 7, 1]
    srcs = [(1 << 40) + (k << 32) for k in range(3)]
    dsts = [(1 << 41) + (k << 32) for k in range(3)]
    a = lambda v: (C.c_uint64 * 3)(*v)
    out = (Entry * 3)()
    cap = 4096
    index = (C.c_uint8 * cap)()
    wide = C.c_uint32(7)
    total = lib.dxtlt_debug_plan_batch(fmt, int(inverse), 2, 1, 0, a(srcs), a(dsts), a(blocks), 3, out, index, cap, C.byref(wide))
    assert total == 64 + (3 + 1) + 1
    assert [(e.first_wg, e.end_wg, e.full_tiles, e.form) for e in out] == [(0, 64, 64, 1), (64, 68, 3, 0), (68, 69, 0, 0)]
    S = bc45_ref.streams(name, True)
    soa = dsts[1] if not inverse else srcs[1]
    mask = 15 if inverse else 63
    assert list(out[1].shift)[:len(S)] == [(soa + off * blocks[1]) & mask for off, w in S]
    assert lib.dxtlt_debug_plan_batch(6, int(inverse), 0, 0, 0, a(srcs), a(dsts), a(blocks), 3, out, index, cap,
                                      C.byref(wide)) == 0xFFFFFFFF
