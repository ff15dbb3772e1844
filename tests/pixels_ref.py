"""CPU statement of the uncompressed-pixel transform, layout version 1 (docs/PIXEL_FORMAT.md), in numpy: forward and inverse
straight from the three definitions -- subtract-green, planes, per-plane delta in segments of 4096 bytes -- plus the
document's worked vectors, the tagged header words and small DDS builders for the tests."""
import ctypes as C
import struct

import numpy as np

INTERLEAVED, PLANAR, PLANAR_DELTA = 0, 1, 2
LAYOUTS = (INTERLEAVED, PLANAR, PLANAR_DELTA)
SEGMENT = 4096
SETTINGS = [(d, l) for d in (False, True) for l in LAYOUTS]

TF_RGBA8888, TF_BGRA8888, TF_BGR888 = 5, 6, 7
VENDOR_TAG, LAYOUT_VERSION = 0xD175, 1


def forward(data, pixel_bytes, decorrelate, layout):
    x = np.asarray(data, dtype=np.uint8)
    B = pixel_bytes
    assert B in (3, 4) and x.size % B == 0 and layout in LAYOUTS
    px = x.reshape(-1, B).copy()
    if decorrelate:
        px[:, 0] -= px[:, 1]      # uint8 arithmetic wraps modulo 256
        px[:, 2] -= px[:, 1]
    if layout == INTERLEAVED:
        return px.reshape(-1)
    planes = np.ascontiguousarray(px.T)      # plane c, pixel i -> byte c * P + i
    if layout == PLANAR_DELTA:
        out = planes.copy()
        out[:, 1:] = planes[:, 1:] - planes[:, :-1]
        out[:, ::SEGMENT] = planes[:, ::SEGMENT]   # the first byte of every segment is stored as it is
        planes = out
    return planes.reshape(-1)


def inverse(data, pixel_bytes, decorrelate, layout):
    x = np.asarray(data, dtype=np.uint8)
    B = pixel_bytes
    assert B in (3, 4) and x.size % B == 0 and layout in LAYOUTS
    P = x.size // B
    if layout == INTERLEAVED:
        px = x.reshape(-1, B).copy()
    else:
        planes = x.reshape(B, P).copy()
        if layout == PLANAR_DELTA:
            for s in range(0, P, SEGMENT):
                planes[:, s:s + SEGMENT] = np.cumsum(planes[:, s:s + SEGMENT], axis=1, dtype=np.uint8)
        px = np.ascontiguousarray(planes.T)
    if decorrelate:
        px[:, 0] += px[:, 1]
        px[:, 2] += px[:, 1]
    return px.reshape(-1)


# ---- the worked vectors of docs/PIXEL_FORMAT.md: three pixels per B, all six settings -------------------------------------
VECTOR_INPUT = {
    4: bytes([10, 200, 30, 255, 12, 201, 29, 254, 250, 5, 0, 7]),
    3: bytes([10, 200, 30, 12, 201, 29, 250, 5, 0]),
}
VECTOR_OUTPUT = {
    (4, False, INTERLEAVED): bytes([10, 200, 30, 255, 12, 201, 29, 254, 250, 5, 0, 7]),
    (4, False, PLANAR): bytes([10, 12, 250, 200, 201, 5, 30, 29, 0, 255, 254, 7]),
    (4, False, PLANAR_DELTA): bytes([10, 2, 238, 200, 1, 60, 30, 255, 227, 255, 255, 9]),
    (4, True, INTERLEAVED): bytes([66, 200, 86, 255, 67, 201, 84, 254, 245, 5, 251, 7]),
    (4, True, PLANAR): bytes([66, 67, 245, 200, 201, 5, 86, 84, 251, 255, 254, 7]),
    (4, True, PLANAR_DELTA): bytes([66, 1, 178, 200, 1, 60, 86, 254, 167, 255, 255, 9]),
    (3, False, INTERLEAVED): bytes([10, 200, 30, 12, 201, 29, 250, 5, 0]),
    (3, False, PLANAR): bytes([10, 12, 250, 200, 201, 5, 30, 29, 0]),
    (3, False, PLANAR_DELTA): bytes([10, 2, 238, 200, 1, 60, 30, 255, 227]),
    (3, True, INTERLEAVED): bytes([66, 200, 86, 67, 201, 84, 245, 5, 251]),
    (3, True, PLANAR): bytes([66, 67, 245, 200, 201, 5, 86, 84, 251]),
    (3, True, PLANAR_DELTA): bytes([66, 1, 178, 200, 1, 60, 86, 254, 167]),
}


# ---- TransformHeader words -------------------------------------------------------------------------------------------------
def header_word(code, decorrelate, layout):
    """bits 0-3 the format code; data bits: 0-1 upstream's version 0, 2 decorrelate, 4..3 layout, 11..5 layout version, 27..12 tag"""
    data = (VENDOR_TAG << 12) | (LAYOUT_VERSION << 5) | (layout << 3) | (int(bool(decorrelate)) << 2)
    return code | (data << 4)


def triple_of(decorrelate, layout):
    """(decorrelation_mode, split_alpha_endpoints, split_colour_endpoints) that the generic entry points read as these settings"""
    return (1 if decorrelate else 0), layout == PLANAR_DELTA, layout != INTERLEAVED


# ---- synthetic DDS files -----------------------------------------------------------------------------------------------------
def mip_pixels(w, h, mips):
    total = 0
    for _ in range(mips):
        total += w * h
        w, h = max(1, w // 2), max(1, h // 2)
    return total


def _dds_header(w, h, mips, pf_flags, fourcc, bits, masks):
    hdr = bytearray(128)
    hdr[0:4] = b"DDS "
    struct.pack_into("<I", hdr, 4, 124)
    struct.pack_into("<I", hdr, 0x08, 0x1007 | (0x20000 if mips > 1 else 0))
    struct.pack_into("<II", hdr, 0x0C, h, w)
    struct.pack_into("<I", hdr, 0x1C, mips)
    struct.pack_into("<I", hdr, 0x4C, 32)
    struct.pack_into("<I", hdr, 0x50, pf_flags)
    hdr[0x54:0x58] = fourcc
    struct.pack_into("<I", hdr, 0x58, bits)
    struct.pack_into("<IIII", hdr, 0x5C, *masks)
    return bytes(hdr)


def dds_dx10(payload, w, h, dxgi, mips=1):
    """DX10 header (148 bytes) in front of `payload`: DXGI 28 = RGBA8888, 87 = BGRA8888, 71 = BC1"""
    dx10 = struct.pack("<IIIII", dxgi, 3, 0, 1, 0)
    return _dds_header(w, h, mips, 0x4, b"DX10", 0, (0, 0, 0, 0)) + dx10 + bytes(payload)


def dds_legacy(payload, w, h, kind, mips=1):
    """legacy pixel-format masks (128 bytes): kind 'rgba', 'bgra' or 'bgr'"""
    if kind == "rgba":
        flags, bits, masks = 0x41, 32, (0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000)
    elif kind == "bgra":
        flags, bits, masks = 0x41, 32, (0x00FF0000, 0x0000FF00, 0x000000FF, 0xFF000000)
    else:
        flags, bits, masks = 0x40, 24, (0x00FF0000, 0x0000FF00, 0x000000FF, 0)
    return _dds_header(w, h, mips, flags, b"\0\0\0\0", bits, masks) + bytes(payload)


# ---- the C symbols the tests call ----------------------------------------------------------------------------------------------
class DdsBatchItem(C.Structure):
    _fields_ = [("input", C.c_void_p), ("input_len", C.c_size_t), ("output", C.c_void_p), ("output_len", C.c_size_t),
                ("decorrelation_mode", C.c_uint8), ("split_alpha_endpoints", C.c_bool), ("split_colour_endpoints", C.c_bool),
                ("status", C.c_int32)]


MAX_SIZE_FN = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))
ESTIMATE_FN = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))


class Estimator(C.Structure):
    """DltSizeEstimator (include/dlt_size_estimator.h)"""
    _fields_ = [("Context", C.c_void_p), ("MaxCompressedSize", MAX_SIZE_FN), ("EstimateCompressedSize", ESTIMATE_FN)]


def counting_estimator():
    """(estimator, calls): an estimator that answers `len` and counts every callback in calls[0]; keep both alive"""
    calls = [0]

    def max_size(_ctx, n, out):
        calls[0] += 1
        out[0] = 0
        return 0

    def estimate(_ctx, _inp, n, _out, _out_len, out):
        calls[0] += 1
        out[0] = n
        return 0

    return Estimator(None, MAX_SIZE_FN(max_size), ESTIMATE_FN(estimate)), calls


def declare(l):
    """argument types of every symbol these tests call: a missing symbol raises AttributeError here, a failure"""
    vp, sz, b, i32, u8, u32, u64 = C.c_void_p, C.c_size_t, C.c_bool, C.c_int32, C.c_uint8, C.c_uint32, C.c_uint64
    for n in ("dxtlt_transform_pixels", "dxtlt_untransform_pixels"):
        getattr(l, n).argtypes, getattr(l, n).restype = [vp, vp, sz, i32, b, u8], i32
    for n in ("dxtlt_transform_pixels_device", "dxtlt_untransform_pixels_device"):
        getattr(l, n).argtypes, getattr(l, n).restype = [vp, vp, sz, i32, b, u8, vp], i32
    l.dxtlt_transform_pixels_range_device.argtypes = [i32, b, vp, vp, u64, u64, u64, b, u8, vp]
    l.dxtlt_transform_pixels_range_device.restype = i32
    l.dxtlt_transform_sharded.argtypes, l.dxtlt_transform_sharded.restype = [i32, b, vp, vp, sz, u8, b, b, i32], i32
    l.dxtlt_file_formats_enable_pixels.argtypes, l.dxtlt_file_formats_enable_pixels.restype = [b], None
    l.dxtlt_transform_header_pack_pixels.argtypes, l.dxtlt_transform_header_pack_pixels.restype = [i32, b, u8], u32
    l.dxtlt_transform_header_unpack_reserved_format.argtypes = [u32, C.POINTER(i32), C.POINTER(b)]
    l.dxtlt_transform_header_unpack_reserved_format.restype = i32
    l.dxtlt_dds_transform.argtypes, l.dxtlt_dds_transform.restype = [vp, sz, vp, sz, u8, b, b], i32
    l.dxtlt_dds_transform_auto.argtypes, l.dxtlt_dds_transform_auto.restype = [vp, sz, vp, sz, C.POINTER(Estimator), b], i32
    l.dxtlt_dds_untransform.argtypes, l.dxtlt_dds_untransform.restype = [vp, sz, vp, sz], i32
    l.dxtlt_dds_transform_batch.argtypes, l.dxtlt_dds_transform_batch.restype = [C.POINTER(DdsBatchItem), sz, b], sz
    return l
