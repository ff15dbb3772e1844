"""The BC6H (UF16) decoder (docs/IMAGE_DECODE.md, "BC6H blocks to a row-major RGBA16F image"), everything that needs no GPU.
Three statements of it meet here: Pillow's decoder, which is independent of this project -- its 8-bit answers recorded in
tests/golden/bc6h_decode_vectors.npz and asked live where Pillow is installed --; the numpy statement of
tests/bc6h_decode_ref.py; and csrc/bc6h_decode.h, the code the kernels run, built for the host through
tests/cpp/bc6h_decode_shim.cpp and called through dxtlt_decode_bc6h_blocks.  Pillow answers in 8 bits, so it pins the fields,
the deltas, the partitions and the interpolation but not the low bits of a half: those are pinned by the worked vectors of the
document, which the numpy statement and the header meet exactly.  The reserved mode values are outside the Pillow comparisons."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bc6h_decode_ref as ref
import bc6h_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "dxt-lossless-transform_amd", "csrc")
OK, E_LENGTH, E_ARGUMENT = 0, 1, 2


@pytest.fixture(scope="module")
def vectors():
    with np.load(os.path.join(GOLDEN, "bc6h_decode_vectors.npz")) as z:
        return z["blocks"], z["pixels"]


@pytest.fixture(scope="module")
def random_blocks():
    blocks = ref.mode_balanced_blocks(200_000, 7)
    return blocks, ref.records(ref.decode_blocks(blocks))


@pytest.fixture(scope="module")
def reserved_blocks():
    return ref.reserved_blocks(512, 8)


def fields_of(blocks, k):
    """{(ch, e): values} and the partition of blocks of class k"""
    bits = bc6h_ref._bits(blocks)
    return ({key: bc6h_ref._value(bits, pos) for key, pos in bc6h_ref.FIELDS[k].items()},
            bc6h_ref._value(bits, bc6h_ref.PARTITION[k]) if bc6h_ref.two_region(k) else None,
            bc6h_ref._value(bits, list(range(bc6h_ref.INDEX_START[k], 128))))


def test_fixture_covers_what_it_promises(vectors):
    blocks, pixels = vectors
    n = blocks.shape[0]
    assert pixels.shape == (n, 16, 3) and pixels.dtype == np.uint8
    assert os.path.getsize(os.path.join(GOLDEN, "bc6h_decode_vectors.npz")) < 200 << 10
    cls = ref.block_classes(blocks)
    assert (cls < 14).all()   # no reserved block
    for k in range(14):
        b = blocks[cls == k]
        fields, part, index = fields_of(b, k)
        if bc6h_ref.two_region(k):
            assert (np.bincount(part, minlength=32) >= 3).all(), k        # every partition
        full = np.stack([v == (1 << bc6h_ref.field_width(k, *key)) - 1 for key, v in fields.items()]).all(axis=0)
        zero = np.stack([v == 0 for v in fields.values()]).all(axis=0)
        assert full.sum() >= 2 and zero.sum() >= 2, k                       # all-ones and all-zero endpoint fields
        width = 128 - bc6h_ref.INDEX_START[k]
        assert (index == 0).sum() >= 4 and (index == (1 << width) - 1).sum() >= 4, k   # every pixel shows e0 / e1 unmixed
        assert b.shape[0] >= 100, k
    # at least half of Pillow's channels are strictly inside its range: a saturated one pins nothing beyond the sign of an error
    share = ((pixels > 0) & (pixels < 255)).mean()
    print("share of the fixture's channels strictly between 0 and 255: %.3f" % share)
    assert share >= 0.5


def test_numpy_statement_is_within_one_of_the_recorded_pillow_answers(vectors):
    blocks, pixels = vectors
    got = ref.pillow_8bit(ref.decode_blocks(blocks)[:, :, :3])
    diff = np.abs(got.astype(np.int64) - pixels.astype(np.int64))
    print("largest difference %d, equal channels %.4f" % (diff.max(), (diff == 0).mean()))
    wrong = np.nonzero((diff > 1).any(axis=(1, 2)))[0]
    assert wrong.size == 0, (wrong[:8], ref.block_classes(blocks[wrong[:8]]))
    assert (ref.decode_blocks(blocks)[:, :, 3] == 0x3C00).all()


def test_numpy_statement_is_within_one_of_live_pillow_on_mode_balanced_blocks():
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow does not import: the live comparison with its BC6H decoder is left out (the recorded one ran)")
    import io

    blocks = ref.mode_balanced_blocks(20_000, 11)
    cls = ref.block_classes(blocks)
    assert (cls < 14).all() and np.bincount(cls, minlength=14).min() > 1200
    n = blocks.shape[0]
    image = Image.open(io.BytesIO(bc6h_ref.dds_dx10(blocks.tobytes(), 4 * n, 4, dxgi=95))).convert("RGB")
    want = np.asarray(image, dtype=np.uint8).reshape(4, n, 4, 3).transpose(1, 0, 2, 3).reshape(n, 16, 3)
    got = ref.pillow_8bit(ref.decode_blocks(blocks)[:, :, :3])
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print("largest difference %d, equal channels %.4f" % (diff.max(), (diff == 0).mean()))
    wrong = np.nonzero((diff > 1).any(axis=(1, 2)))[0]
    assert wrong.size == 0, (wrong[:8], cls[wrong[:8]])
    # an image whose sides are no multiples of 4, in Pillow's block order
    w, h = 37, 22
    m = ((w + 3) // 4) * ((h + 3) // 4)
    odd = np.asarray(Image.open(io.BytesIO(bc6h_ref.dds_dx10(blocks[:m].tobytes(), w, h, dxgi=95))).convert("RGB"), dtype=np.uint8)
    mine = ref.pillow_8bit(ref.image_of(ref.decode_blocks(blocks[:m]), w, h)[:, :, :3])
    assert np.abs(mine.astype(np.int64) - odd.astype(np.int64)).max() <= 1


def test_reserved_blocks_decode_to_black_in_the_numpy_statement(reserved_blocks):
    px = ref.decode_blocks(reserved_blocks)
    assert not px[:, :, :3].any() and (px[:, :, 3] == 0x3C00).all()


# ---- the worked vectors of the document: the low bits of a half ----------------------------------------------------------------
# per base width: (field value, unquantised, final half) for 0, 1, the middle value and all ones
ENDPOINT_VECTORS = {
    6: ((0, 0x0000, 0x0000), (1, 0x0600, 0x02E8), (32, 0x8200, 0x3EF8), (63, 0xFFFF, 0x7BFF)),
    7: ((0, 0x0000, 0x0000), (1, 0x0300, 0x0174), (64, 0x8100, 0x3E7C), (127, 0xFFFF, 0x7BFF)),
    8: ((0, 0x0000, 0x0000), (1, 0x0180, 0x00BA), (128, 0x8080, 0x3E3E), (255, 0xFFFF, 0x7BFF)),
    9: ((0, 0x0000, 0x0000), (1, 0x00C0, 0x005D), (256, 0x8040, 0x3E1F), (511, 0xFFFF, 0x7BFF)),
    10: ((0, 0x0000, 0x0000), (1, 0x0060, 0x002E), (512, 0x8020, 0x3E0F), (1023, 0xFFFF, 0x7BFF)),
    11: ((0, 0x0000, 0x0000), (1, 0x0030, 0x0017), (1024, 0x8010, 0x3E07), (2047, 0xFFFF, 0x7BFF)),
    12: ((0, 0x0000, 0x0000), (1, 0x0018, 0x000B), (2048, 0x8008, 0x3E03), (4095, 0xFFFF, 0x7BFF)),
    16: ((0, 0x0000, 0x0000), (1, 0x0001, 0x0000), (32768, 0x8000, 0x3E00), (65535, 0xFFFF, 0x7BFF)),
}
CLASSES_OF_WIDTH = {6: (9,), 7: (1,), 8: (6, 7, 8), 9: (5,), 10: (0, 10), 11: (2, 3, 4, 11), 12: (12,), 16: (13,)}

# One region: class 11 (11-bit base, 9-bit deltas); red w = 1935, x = 320 (-192: 1743); green 100, 5 (105); blue 2047, 1 (wraps
# to 0); pixel i has index i.  Unquantised: red 61936 / 55792, green 3216 / 3376, blue 65535 / 0.
ONE_REGION = dict(k=11, ep={(0, 0): 1935, (0, 1): 320, (1, 0): 100, (1, 1): 5, (2, 0): 2047, (2, 1): 1}, partition=0,
                  index_bits=0x7F6E5D4C3B2A1908,
                  pixels=[[30000, 1557, 31743], [29814, 1562, 29759], [29581, 1568, 27279], [29395, 1573, 25295], [29209, 1578, 23311],
                          [29023, 1583, 21327], [28791, 1589, 18847], [28605, 1594, 16863], [28419, 1598, 14880], [28233, 1603, 12896],
                          [28000, 1610, 10416], [27814, 1614, 8432], [27628, 1619, 6448], [27442, 1624, 4464], [27210, 1630, 1984],
                          [27024, 1635, 0]])
# Two regions: class 1 (7-bit base, 6-bit deltas), partition 13 (pixels 8..15 are subset 1, its anchor pixel 15); red w = 40,
# x y z = 3, 61 (-3), 0: 43, 37, 40; green 100 and 60 (-4), 2, 33 (-31): 96, 102, 69; blue 127 and 1, 63 (-1), 32 (-32): 0 (wrapped),
# 126, 95; pixel i has index i % 8, pixel 15 (an anchor) index 3.
TWO_REGIONS = dict(k=1, ep={(0, 0): 40, (0, 1): 3, (0, 2): 61, (0, 3): 0, (1, 0): 100, (1, 1): 60, (1, 2): 2, (1, 3): 33,
                            (2, 0): 127, (2, 1): 1, (2, 2): 63, (2, 3): 32}, partition=13, index_bits=0x3D63447D6344,
                   pixels=[[10044, 24924, 31743], [10148, 24784, 27279], [10253, 24645, 22815], [10357, 24505, 18351], [10474, 24350, 13392],
                           [10578, 24211, 8928], [10683, 24071, 4464], [10788, 23932, 0], [9300, 25420, 31372], [9404, 24269, 30290],
                           [9509, 23118, 29209], [9613, 21967, 28128], [9730, 20688, 26927], [9834, 19537, 25846], [9939, 18386, 24765],
                           [9613, 21967, 28128]])


def worked_vectors():
    """(blocks, (n, 16, 4) expected halves)"""
    blocks, want = [], []
    for bits, rows in ENDPOINT_VECTORS.items():
        for k in CLASSES_OF_WIDTH[bits]:
            assert bc6h_ref.WIDTHS[k][0] == bits
            for value, _, half in rows:
                # every endpoint is `value`: the deltas 0 in the transformed modes, the value itself in the others; random indices
                ep = {(ch, e): value if e == 0 or not bc6h_ref.TRANSFORMED[k] else 0 for ch in range(3) for e in range(bc6h_ref.n_endpoints(k))}
                blocks.append(bc6h_ref.pack_block(k, ep, 21, 0x2DB6C924B6DB1A5F))
                want.append(np.tile(np.array([half, half, half, 0x3C00], dtype=np.uint16), (16, 1)))
    for case in (ONE_REGION, TWO_REGIONS):
        blocks.append(bc6h_ref.pack_block(case["k"], case["ep"], case["partition"], case["index_bits"]))
        want.append(np.concatenate([np.array(case["pixels"], dtype=np.uint16), np.full((16, 1), 0x3C00, dtype=np.uint16)], axis=1))
    return np.stack(blocks), np.stack(want)


def test_the_worked_vectors_follow_from_the_definition():
    """the table's own arithmetic: unquantised and final value of every row from the two formulas"""
    for bits, rows in ENDPOINT_VECTORS.items():
        assert [v for v, _, _ in rows] == [0, 1, 1 << (bits - 1), (1 << bits) - 1]
        for value, unq, half in rows:
            want = value if bits >= 15 else 0 if value == 0 else 0xFFFF if value == (1 << bits) - 1 else ((value << 16) + 0x8000) >> bits
            assert unq == want and half == (unq * 31) >> 6, (bits, value)


def test_numpy_statement_equals_the_worked_vectors_exactly():
    blocks, want = worked_vectors()
    assert np.array_equal(ref.decode_blocks(blocks), want)


# ---- csrc/bc6h_decode.h on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "bc6h_decode_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "bc6h_decode_shim.cpp")])
    l = C.CDLL(so)
    l.shim_bc6h_decode_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    l.shim_bc6h_decode_blocks.restype = None
    l.shim_bc6h_field_runs.argtypes = [C.c_int, C.c_void_p, C.c_int]
    l.shim_bc6h_class_desc.argtypes = [C.c_int, C.c_void_p]
    return l


@pytest.fixture(scope="module")
def shim(shim_lib):
    def decode(blocks):
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
        out = np.full((blocks.shape[0], 128), 0xA5, dtype=np.uint8)
        shim_lib.shim_bc6h_decode_blocks(blocks.ctypes.data, out.ctypes.data, blocks.shape[0])
        return out

    return decode


@pytest.fixture(scope="module")
def host_call(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    l.dxtlt_decode_bc6h_blocks.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    l.dxtlt_decode_bc6h_blocks.restype = C.c_int32

    def decode(blocks):
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
        out = np.full((blocks.shape[0], 128), 0xA5, dtype=np.uint8)
        assert l.dxtlt_decode_bc6h_blocks(blocks.ctypes.data, blocks.size, out.ctypes.data, out.size) == OK
        return out

    decode.lib = l
    return decode


def check_decoder(decode, vectors, random_blocks, reserved_blocks):
    blocks, want = worked_vectors()
    assert np.array_equal(decode(blocks), ref.records(want)), "the worked vectors"
    blocks, _ = vectors
    assert np.array_equal(decode(blocks), ref.records(ref.decode_blocks(blocks))), "the fixture"
    blocks, want = random_blocks
    got = decode(blocks)
    wrong = np.nonzero((got != want).any(axis=1))[0]
    assert wrong.size == 0, (wrong[:8], ref.block_classes(blocks[wrong[:8]]))
    black = np.tile(np.array([0, 0, 0, 0x3C00], dtype="<u2"), 16).view(np.uint8)
    assert (decode(reserved_blocks) == black).all(), "reserved blocks are black"
    mixed = ref.interleaved_class_blocks(900, 9)
    assert np.array_equal(decode(mixed), ref.records(ref.decode_blocks(mixed)))


def test_the_header_on_the_host_equals_the_numpy_statement(shim, vectors, random_blocks, reserved_blocks):
    check_decoder(shim, vectors, random_blocks, reserved_blocks)


def test_the_host_call_equals_the_numpy_statement(host_call, vectors, random_blocks, reserved_blocks):
    check_decoder(host_call, vectors, random_blocks, reserved_blocks)


def test_the_headers_field_table_is_the_layout_strings(shim_lib):
    """csrc/bc6h_decode_fields.h, as compiled: every class's runs put exactly the block bits of tests/bc6h_ref.py LAYOUTS at the
    value bits of their fields, and its widths, delta flag and region count are that module's"""
    for k in range(14):
        desc = np.zeros(6, dtype=np.int32)
        assert shim_lib.shim_bc6h_class_desc(k, desc.ctypes.data) == 0
        assert tuple(desc[:4]) == bc6h_ref.WIDTHS[k] and bool(desc[4]) == bc6h_ref.TRANSFORMED[k] and bool(desc[5]) == bc6h_ref.two_region(k)
        runs = np.zeros((64, 5), dtype=np.int32)
        n = shim_lib.shim_bc6h_field_runs(k, runs.ctypes.data, 64)
        assert 0 < n <= 64
        got = {}
        for ch, e, src, dst, length in runs[:n].tolist():
            for i in range(length):
                assert (ch, e, dst + i) not in got, (k, ch, e, dst + i)
                got[(ch, e, dst + i)] = src + i
        want = {(ch, e, i): p for (ch, e), pos in bc6h_ref.FIELDS[k].items() for i, p in enumerate(pos)}
        assert got == want, k
    assert shim_lib.shim_bc6h_class_desc(14, None) == -1


def test_the_field_header_holds_what_its_generator_prints():
    text = open(os.path.join(CSRC, "bc6h_decode_fields.h")).read()
    m = re.search(r"// ---- GENERATED by tests/bc6h_decode_ref.py decode_field_table\(\) ----\n(.*?)// ---- end of GENERATED ----", text, re.S)
    assert m and m.group(1) == ref.decode_field_table()


def test_the_block_calls_check_their_lengths_as_the_bc7_calls_do(host_call):
    l = host_call.lib
    l.dxtlt_decode_bc6h_blocks_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    l.dxtlt_decode_bc6h_blocks_device.restype = C.c_int32
    src, dst = 0x7F1000000000, 0x7F2000000000   # made up, never dereferenced
    for call in (lambda *a: l.dxtlt_decode_bc6h_blocks(*a), lambda *a: l.dxtlt_decode_bc6h_blocks_device(*a, None)):
        assert call(src, 24, dst, 1024) == E_LENGTH
        assert call(None, 24, None, 0) == E_LENGTH        # the length before the pointers
        assert call(None, 32, dst, 256) == E_ARGUMENT
        assert call(src, 32, None, 256) == E_ARGUMENT
        assert call(src, 32, dst, 255) == E_ARGUMENT
        assert call(None, 0, None, 0) == OK


def test_python_module_decodes_host_buffers(pkg, vectors):
    from dxt_lossless_transform_amd import decode

    blocks, _ = vectors
    want = ref.records(ref.decode_blocks(blocks))
    out = np.zeros(want.size, dtype=np.uint8)
    decode.decode_bc6h_blocks(blocks.reshape(-1), out)
    assert np.array_equal(out.reshape(-1, 128), want)
    with pytest.raises(pkg.InvalidLength):
        decode.decode_bc6h_blocks(np.zeros(17, np.uint8), out)
    with pytest.raises(pkg.OutputBufferTooSmall):
        decode.decode_bc6h_blocks(np.zeros(32, np.uint8), np.zeros(255, np.uint8))
