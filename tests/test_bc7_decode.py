"""The BC7 decoder (docs/IMAGE_DECODE.md, "BC7"), everything that needs no GPU.  Three statements of it meet here: Pillow's
decoder, which is independent of this project -- its answers recorded in tests/golden/bc7_decode_vectors.npz (every partition
of every mode, every rotation x index selector, all-zero and all-one endpoints) and asked live where Pillow is installed --;
the numpy statement of tests/bc7_decode_ref.py; and csrc/bc7_decode.h, the code the kernels run, built for the host through
tests/cpp/bc7_decode_shim.cpp and called through dxtlt_decode_bc7_blocks.  The reserved encoding (byte 0 == 0) is the one case
outside the Pillow comparisons: Direct3D specifies zeros for it, Pillow answers opaque black."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import bc7_decode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, E_LENGTH, E_ARGUMENT = 0, 1, 2


@pytest.fixture(scope="module")
def vectors():
    with np.load(os.path.join(GOLDEN, "bc7_decode_vectors.npz")) as z:
        return z["blocks"], z["pixels"]


@pytest.fixture(scope="module")
def random_blocks():
    blocks = ref.mode_balanced_blocks(200_000, 7)
    return blocks, ref.decode_blocks(blocks)


@pytest.fixture(scope="module")
def reserved_blocks():
    blocks = ref.with_mode(np.random.default_rng(8).integers(0, 256, (512, 16), dtype=np.uint8), np.full(512, 8))
    assert (blocks[:, 0] == 0).all() and blocks[:, 1:].any()
    return blocks


def test_fixture_covers_every_mode_partition_rotation_and_selector(vectors):
    blocks, pixels = vectors
    assert blocks.shape == (1710, 16) and pixels.shape == (1710, 64) and os.path.getsize(os.path.join(GOLDEN, "bc7_decode_vectors.npz")) < 200 << 10
    modes = ref.block_modes(blocks)
    assert (modes < 8).all()   # no reserved block
    header_bits = [4, 6, 6, 6, 3, 2, 0, 6]
    for m in range(8):
        b = blocks[modes == m]
        header = (b[:, :4].copy().view("<u4")[:, 0] >> (m + 1)) & ((1 << header_bits[m]) - 1)
        counts = np.bincount(header, minlength=1 << header_bits[m])
        assert (counts >= 6).all(), m   # all-zero and all-one endpoints and four random fills per header value


def test_numpy_statement_equals_the_recorded_pillow_answers(vectors):
    blocks, pixels = vectors
    got = ref.decode_blocks(blocks)
    wrong = np.nonzero((got != pixels).any(axis=1))[0]
    assert wrong.size == 0, (wrong[:8], ref.block_modes(blocks[wrong[:8]]))


def test_numpy_statement_equals_the_recorded_digest_of_a_real_texture():
    digests = json.load(open(os.path.join(GOLDEN, "bc7_decode_digests.json")))
    entry = digests["r2-256-bc7.payload.bin"]
    blocks = np.fromfile(os.path.join(GOLDEN, "r2-256-bc7.payload.bin"), dtype=np.uint8).reshape(-1, 16)
    modes = ref.block_modes(blocks)
    assert blocks.shape[0] == 4096 and set(modes.tolist()) == set(range(8))
    image = ref.image_of(ref.decode_blocks(blocks), entry["width"], entry["height"])
    assert hashlib.sha256(image.tobytes()).hexdigest() == entry["sha256"]


def test_numpy_statement_equals_live_pillow_on_mode_balanced_blocks():
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow does not import: the live comparison with its BC7 decoder is left out (the recorded one ran)")
    blocks = ref.mode_balanced_blocks(20_000, 11)
    modes = ref.block_modes(blocks)
    assert (modes < 8).all() and np.bincount(modes, minlength=8).min() > 2000
    n = blocks.shape[0]
    image = Image.frombytes("RGBA", (4 * n, 4), blocks.tobytes(), "bcn", (7,))
    want = np.frombuffer(image.tobytes(), np.uint8).reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 64)
    got = ref.decode_blocks(blocks)
    wrong = np.nonzero((got != want).any(axis=1))[0]
    assert wrong.size == 0, (wrong[:8], modes[wrong[:8]])
    # an image whose sides are no multiples of 4, in Pillow's block order
    w, h = 37, 22
    m = ((w + 3) // 4) * ((h + 3) // 4)
    odd = np.frombuffer(Image.frombytes("RGBA", (w, h), blocks[:m].tobytes(), "bcn", (7,)).tobytes(), np.uint8).reshape(h, w, 4)
    assert np.array_equal(ref.image_of(got[:m], w, h), odd)


def test_reserved_blocks_decode_to_zeros_in_the_numpy_statement(reserved_blocks):
    assert not ref.decode_blocks(reserved_blocks).any()


# ---- csrc/bc7_decode.h on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "bc7_decode_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "bc7_decode_shim.cpp")])
    l = C.CDLL(so)
    l.shim_bc7_decode_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    l.shim_bc7_decode_blocks.restype = None

    def decode(blocks):
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
        out = np.full((blocks.shape[0], 64), 0xA5, dtype=np.uint8)
        l.shim_bc7_decode_blocks(blocks.ctypes.data, out.ctypes.data, blocks.shape[0])
        return out

    return decode


@pytest.fixture(scope="module")
def host_call(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    l.dxtlt_decode_bc7_blocks.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    l.dxtlt_decode_bc7_blocks.restype = C.c_int32

    def decode(blocks):
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
        out = np.full((blocks.shape[0], 64), 0xA5, dtype=np.uint8)
        assert l.dxtlt_decode_bc7_blocks(blocks.ctypes.data, blocks.size, out.ctypes.data, out.size) == OK
        return out

    decode.lib = l
    return decode


def check_decoder(decode, vectors, random_blocks, reserved_blocks):
    blocks, pixels = vectors
    assert np.array_equal(decode(blocks), pixels), "the recorded Pillow answers"
    blocks, want = random_blocks
    got = decode(blocks)
    wrong = np.nonzero((got != want).any(axis=1))[0]
    assert wrong.size == 0, (wrong[:8], ref.block_modes(blocks[wrong[:8]]))
    assert not decode(reserved_blocks).any(), "reserved blocks are 64 zero bytes"
    mixed = ref.interleaved_class_blocks(900, 9)
    assert np.array_equal(decode(mixed), ref.decode_blocks(mixed))


def test_the_header_on_the_host_equals_the_numpy_statement(shim, vectors, random_blocks, reserved_blocks):
    check_decoder(shim, vectors, random_blocks, reserved_blocks)


def test_the_host_call_equals_the_numpy_statement(host_call, vectors, random_blocks, reserved_blocks):
    check_decoder(host_call, vectors, random_blocks, reserved_blocks)


def test_the_block_calls_check_their_lengths_as_the_bc3_calls_do(host_call):
    l = host_call.lib
    l.dxtlt_decode_bc7_blocks_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    l.dxtlt_decode_bc7_blocks_device.restype = C.c_int32
    src, dst = 0x7F1000000000, 0x7F2000000000   # made up, never dereferenced
    for call in (lambda *a: l.dxtlt_decode_bc7_blocks(*a), lambda *a: l.dxtlt_decode_bc7_blocks_device(*a, None)):
        assert call(src, 24, dst, 1024) == E_LENGTH
        assert call(None, 24, None, 0) == E_LENGTH        # the length before the pointers
        assert call(None, 32, dst, 128) == E_ARGUMENT
        assert call(src, 32, None, 128) == E_ARGUMENT
        assert call(src, 32, dst, 127) == E_ARGUMENT
        assert call(None, 0, None, 0) == OK


def test_python_module_decodes_host_buffers(pkg, vectors):
    from dxt_lossless_transform_amd import decode

    blocks, pixels = vectors
    out = np.zeros(pixels.size, dtype=np.uint8)
    decode.decode_bc7_blocks(blocks.reshape(-1), out)
    assert np.array_equal(out.reshape(-1, 64), pixels)
    with pytest.raises(pkg.InvalidLength):
        decode.decode_bc7_blocks(np.zeros(17, np.uint8), out)
    with pytest.raises(pkg.OutputBufferTooSmall):
        decode.decode_bc7_blocks(np.zeros(32, np.uint8), np.zeros(127, np.uint8))
