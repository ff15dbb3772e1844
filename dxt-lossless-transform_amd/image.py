"""BC1 / BC2 / BC3 blocks -> a row-major RGBA8888 image and BC4 / BC5 blocks -> a row-major R8 / RG8 image, over
include/dxtlt_image.h (docs/IMAGE_DECODE.md).

``decode_image`` decodes a block array in block order; ``untransform_decode_image`` decodes a block range of a TRANSFORMED
buffer in one kernel (the untransformed blocks never touch memory); ``mip_level`` says which range a mip level is.  Pixel
(x, y) is the bytes r, g, b, a at ``y * pitch + 4 * x`` of the output; nothing else of the output is written.
1-D ``uint8`` numpy / bytes-like host buffers or CUDA ``torch.uint8`` tensors (torch's current stream).  No CPU fallback:
``decode_image`` takes device tensors only, ``untransform_decode_image`` both kinds.

``decode_channel_image`` and ``untransform_decode_channel_image`` are the same two calls for ``"bc4"`` / ``"bc5"``: a pixel is
1 / 2 bytes (r, or r, g) at ``y * pitch + bpp * x``, the default pitch ``bpp * width``, the one setting ``split_endpoints``.

``decode_bc7_image`` and ``untransform_decode_bc7_image`` are the two calls for BC7 (include/dxtlt_bc7_image.h): RGBA8888, no
settings, any ``first_block``.  ``decode_bc6h_image`` and ``untransform_decode_bc6h_image`` are the two calls for BC6H
(include/dxtlt_bc6h_image.h): unsigned blocks to RGBA16F, 8 bytes per pixel, the default pitch ``8 * width``.

``untransform_decode_images`` and ``decode_images`` write several images of one buffer in one call, for all five formats: a
region is ``(first_block, width, height)``, and ``mip_chain`` lists the regions of a mip chain.
``untransform_decode_bc7_images`` and ``decode_bc7_images`` are the same two calls for BC7 (no ``fmt``, no settings),
``untransform_decode_bc6h_images`` and ``decode_bc6h_images`` for BC6H (RGBA16F, the default pitch ``8 * width``).
``untransform_decode_images_batch`` does the same for MANY transformed device buffers in one call: one launch per (format,
settings) present in the batch, whatever the number of buffers; ``untransform_decode_bc7_images_batch`` and
``untransform_decode_bc6h_images_batch`` are that call for BC7 and BC6H: at most two launches, whatever the number of buffers."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_FMT = {"bc1": 1, "bc2": 2, "bc3": 3}
_BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16}
_CHANNEL_FMT = {"bc4": 4, "bc5": 5}
_CHANNEL_BLOCK = {"bc4": 8, "bc5": 16}
_CHANNEL_BPP = {"bc4": 1, "bc5": 2}
_ALL_FMT = {**_FMT, **_CHANNEL_FMT}
_ALL_BLOCK = {**_BLOCK, **_CHANNEL_BLOCK}
_ALL_BPP = {"bc1": 4, "bc2": 4, "bc3": 4, **_CHANNEL_BPP}
_REGION_BLOCK = {**_ALL_BLOCK, "bc7": 16, "bc6h": 16}   # the region helpers serve the BC7 and BC6H calls too, which have entry points of their own
_REGION_BPP = {**_ALL_BPP, "bc7": 4, "bc6h": 8}
_declared = False


class ImageBatchItem(C.Structure):   # DxtltImageBatchItem, include/dxtlt_image.h
    _fields_ = [("d_transformed", C.c_void_p), ("total_blocks", C.c_uint64), ("regions", C.c_void_p), ("region_count", C.c_uint32),
                ("format", C.c_uint8), ("decorrelation_mode", C.c_uint8), ("split_alpha_endpoints", C.c_uint8),
                ("split_colour_endpoints", C.c_uint8)]


class Bc7ImageBatchItem(C.Structure):   # DxtltBc7ImageBatchItem, include/dxtlt_bc7_image.h
    _fields_ = [("d_transformed", C.c_void_p), ("total_blocks", C.c_uint64), ("regions", C.c_void_p), ("region_count", C.c_uint32),
                ("reserved", C.c_uint32)]


class Bc6hImageBatchItem(C.Structure):   # DxtltBc6hImageBatchItem, include/dxtlt_bc6h_image.h
    _fields_ = list(Bc7ImageBatchItem._fields_)


class ImageRegion(C.Structure):   # DxtltImageRegion, include/dxtlt_image.h
    _fields_ = [("first_block", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("pixels", C.c_void_p),
                ("pitch", C.c_uint64)]


def _l():
    global _declared
    l = _lib.load()
    if not _declared:
        vp, i32, u32, u64, u8, b = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint8, C.c_bool
        l.dxtlt_decode_image_device.argtypes = [i32, vp, u32, u32, vp, u64, vp]
        l.dxtlt_untransform_decode_image_device.argtypes = [i32, vp, u64, u64, u32, u32, u8, b, b, vp, u64, vp]
        l.dxtlt_untransform_decode_image.argtypes = [i32, vp, C.c_size_t, u64, u32, u32, u8, b, b, vp, u64]
        l.dxtlt_image_mip_level.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64),
                                            C.POINTER(u64)]
        l.dxtlt_decode_channel_image_device.argtypes = [i32, vp, u32, u32, vp, u64, vp]
        l.dxtlt_untransform_decode_channel_image_device.argtypes = [i32, vp, u64, u64, u32, u32, b, vp, u64, vp]
        l.dxtlt_untransform_decode_channel_image.argtypes = [i32, vp, C.c_size_t, u64, u32, u32, b, vp, u64]
        rp = C.POINTER(ImageRegion)
        l.dxtlt_untransform_decode_images_device.argtypes = [i32, vp, u64, rp, C.c_size_t, u8, b, b, vp]
        l.dxtlt_decode_images_device.argtypes = [i32, vp, u64, rp, C.c_size_t, vp]
        l.dxtlt_untransform_decode_images.argtypes = [i32, vp, C.c_size_t, rp, C.c_size_t, u8, b, b]
        l.dxtlt_image_mip_chain.argtypes = [u32, u32, u32, u64, rp, C.POINTER(u64)]
        l.dxtlt_untransform_decode_images_batch_device.argtypes = [C.POINTER(ImageBatchItem), C.c_size_t, vp]
        l.dxtlt_decode_bc7_image_device.argtypes = [vp, u32, u32, vp, u64, vp]
        l.dxtlt_untransform_decode_bc7_image_device.argtypes = [vp, u64, u64, u32, u32, vp, u64, vp]
        l.dxtlt_untransform_decode_bc7_image.argtypes = [vp, C.c_size_t, u64, u32, u32, vp, u64]
        l.dxtlt_untransform_decode_bc7_images_device.argtypes = [vp, u64, rp, C.c_size_t, vp]
        l.dxtlt_decode_bc7_images_device.argtypes = [vp, u64, rp, C.c_size_t, vp]
        l.dxtlt_untransform_decode_bc7_images.argtypes = [vp, C.c_size_t, rp, C.c_size_t]
        l.dxtlt_untransform_decode_bc7_images_batch_device.argtypes = [C.POINTER(Bc7ImageBatchItem), C.c_size_t, vp]
        l.dxtlt_decode_bc6h_image_device.argtypes = [vp, u32, u32, vp, u64, vp]
        l.dxtlt_untransform_decode_bc6h_image_device.argtypes = [vp, u64, u64, u32, u32, vp, u64, vp]
        l.dxtlt_untransform_decode_bc6h_image.argtypes = [vp, C.c_size_t, u64, u32, u32, vp, u64]
        l.dxtlt_untransform_decode_bc6h_images_device.argtypes = [vp, u64, rp, C.c_size_t, vp]
        l.dxtlt_decode_bc6h_images_device.argtypes = [vp, u64, rp, C.c_size_t, vp]
        l.dxtlt_untransform_decode_bc6h_images.argtypes = [vp, C.c_size_t, rp, C.c_size_t]
        l.dxtlt_untransform_decode_bc6h_images_batch_device.argtypes = [C.POINTER(Bc6hImageBatchItem), C.c_size_t, vp]
        for f in (l.dxtlt_decode_bc6h_image_device, l.dxtlt_untransform_decode_bc6h_image_device, l.dxtlt_untransform_decode_bc6h_image,
                  l.dxtlt_untransform_decode_bc6h_images_device, l.dxtlt_decode_bc6h_images_device, l.dxtlt_untransform_decode_bc6h_images,
                  l.dxtlt_untransform_decode_bc6h_images_batch_device):
            f.restype = i32
        for f in (l.dxtlt_decode_bc7_image_device, l.dxtlt_untransform_decode_bc7_image_device, l.dxtlt_untransform_decode_bc7_image,
                  l.dxtlt_untransform_decode_bc7_images_device, l.dxtlt_decode_bc7_images_device, l.dxtlt_untransform_decode_bc7_images,
                  l.dxtlt_untransform_decode_bc7_images_batch_device):
            f.restype = i32
        for f in (l.dxtlt_untransform_decode_images_device, l.dxtlt_decode_images_device, l.dxtlt_untransform_decode_images,
                  l.dxtlt_image_mip_chain, l.dxtlt_untransform_decode_images_batch_device):
            f.restype = i32
        for f in (l.dxtlt_decode_image_device, l.dxtlt_untransform_decode_image_device, l.dxtlt_untransform_decode_image,
                  l.dxtlt_image_mip_level, l.dxtlt_decode_channel_image_device, l.dxtlt_untransform_decode_channel_image_device,
                  l.dxtlt_untransform_decode_channel_image):
            f.restype = i32
        _declared = True
    return l


def _check(rc: int) -> None:
    from . import DeviceError

    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())


def image_blocks(width: int, height: int) -> int:
    return ((width + 3) // 4) * ((height + 3) // 4)


def mip_level(width: int, height: int, mip_count: int, level: int):
    """(level_width, level_height, first_block, num_blocks, total_blocks) of level ``level`` of a ``width`` x ``height``
    texture whose ``mip_count`` levels are stored largest first.  No device needed."""
    w, h = C.c_uint32(), C.c_uint32()
    first, num, total = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(_l().dxtlt_image_mip_level(width, height, mip_count, level, C.byref(w), C.byref(h), C.byref(first), C.byref(num),
                                      C.byref(total)))
    return w.value, h.value, first.value, num.value, total.value


def _output(src, width, height, out, pitch, bpp=4):
    """the output buffer (a new one on the source's side when ``out`` is None), its _Buf and the pitch"""
    from . import OutputBufferTooSmall, _Buf

    if pitch is None:
        pitch = bpp * width
    need = pitch * (height - 1) + bpp * width if width and height else 0
    if out is None:
        if src.device is None:
            out = np.zeros(pitch * height, dtype=np.uint8)
        else:
            import torch

            out = torch.zeros(pitch * height, dtype=torch.uint8, device=f"cuda:{src.device}")
    dst = _Buf(out, True)
    if dst.device != src.device:
        raise TypeError("all buffers must be host buffers or all be tensors on one device")
    if dst.nbytes < need:
        raise OutputBufferTooSmall(need, dst.nbytes)
    return out, dst, pitch


def decode_image(fmt: str, blocks, width: int, height: int, out=None, pitch=None):
    """``blocks``: ceil(width / 4) * ceil(height / 4) blocks in block order, a CUDA tensor.  Returns ``out`` (a new tensor of
    ``pitch * height`` bytes when None); ``pitch`` defaults to ``4 * width``."""
    from . import InvalidLength, _Buf

    src = _Buf(blocks, False)
    if src.device is None:
        raise TypeError("decode_image takes device tensors (the library has no host-pointer form of it)")
    if src.nbytes < image_blocks(width, height) * _BLOCK[fmt]:
        raise InvalidLength(src.nbytes)
    out, dst, pitch = _output(src, width, height, out, pitch)
    import torch

    with torch.cuda.device(src.device):
        _check(_l().dxtlt_decode_image_device(_FMT[fmt], src.ptr, width, height, dst.ptr, pitch,
                                              torch.cuda.current_stream(src.device).cuda_stream))
    return out


def untransform_decode_image(fmt: str, transformed, width: int, height: int, *, first_block: int = 0, total_blocks=None,
                             decorrelation_mode, split_alpha_endpoints: bool, split_colour_endpoints: bool, out=None, pitch=None):
    """``transformed``: the WHOLE transformed buffer of ``total_blocks`` blocks (default: its length); the image is its blocks
    [first_block, first_block + ceil(width / 4) * ceil(height / 4)).  Returns ``out``."""
    from . import InvalidLength, _Buf

    src = _Buf(transformed, False)
    if src.nbytes % _BLOCK[fmt] != 0:
        raise InvalidLength(src.nbytes)
    if total_blocks is None:
        total_blocks = src.nbytes // _BLOCK[fmt]
    if total_blocks * _BLOCK[fmt] > src.nbytes:
        raise InvalidLength(src.nbytes)
    out, dst, pitch = _output(src, width, height, out, pitch)
    mode, sa, sc = int(decorrelation_mode), bool(split_alpha_endpoints), bool(split_colour_endpoints)
    l = _l()
    if src.device is None:
        _check(l.dxtlt_untransform_decode_image(_FMT[fmt], src.ptr, total_blocks * _BLOCK[fmt], first_block, width, height, mode,
                                                sa, sc, dst.ptr, pitch))
        return out
    import torch

    with torch.cuda.device(src.device):
        _check(l.dxtlt_untransform_decode_image_device(_FMT[fmt], src.ptr, total_blocks, first_block, width, height, mode, sa, sc,
                                                       dst.ptr, pitch, torch.cuda.current_stream(src.device).cuda_stream))
    return out


def decode_channel_image(fmt: str, blocks, width: int, height: int, out=None, pitch=None):
    """``fmt``: ``"bc4"`` / ``"bc5"``.  ``blocks``: ceil(width / 4) * ceil(height / 4) blocks in block order, a CUDA tensor.
    Returns ``out`` (a new tensor of ``pitch * height`` bytes when None); ``pitch`` defaults to ``bpp * width``."""
    from . import InvalidLength, _Buf

    code, bpp = _CHANNEL_FMT[fmt], _CHANNEL_BPP[fmt]
    src = _Buf(blocks, False)
    if src.device is None:
        raise TypeError("decode_channel_image takes device tensors (the library has no host-pointer form of it)")
    if src.nbytes < image_blocks(width, height) * _CHANNEL_BLOCK[fmt]:
        raise InvalidLength(src.nbytes)
    out, dst, pitch = _output(src, width, height, out, pitch, bpp)
    import torch

    with torch.cuda.device(src.device):
        _check(_l().dxtlt_decode_channel_image_device(code, src.ptr, width, height, dst.ptr, pitch,
                                                      torch.cuda.current_stream(src.device).cuda_stream))
    return out


def untransform_decode_channel_image(fmt: str, transformed, width: int, height: int, *, first_block: int = 0, total_blocks=None,
                                     split_endpoints: bool, out=None, pitch=None):
    """``fmt``: ``"bc4"`` / ``"bc5"``.  ``transformed``: the WHOLE transformed buffer of ``total_blocks`` blocks (default: its
    length); the image is its blocks [first_block, first_block + ceil(width / 4) * ceil(height / 4)).  Returns ``out``."""
    from . import InvalidLength, _Buf

    code, bs = _CHANNEL_FMT[fmt], _CHANNEL_BLOCK[fmt]
    src = _Buf(transformed, False)
    if src.nbytes % bs != 0:
        raise InvalidLength(src.nbytes)
    if total_blocks is None:
        total_blocks = src.nbytes // bs
    if total_blocks * bs > src.nbytes:
        raise InvalidLength(src.nbytes)
    out, dst, pitch = _output(src, width, height, out, pitch, _CHANNEL_BPP[fmt])
    l = _l()
    if src.device is None:
        _check(l.dxtlt_untransform_decode_channel_image(code, src.ptr, total_blocks * bs, first_block, width, height,
                                                        bool(split_endpoints), dst.ptr, pitch))
        return out
    import torch

    with torch.cuda.device(src.device):
        _check(l.dxtlt_untransform_decode_channel_image_device(code, src.ptr, total_blocks, first_block, width, height,
                                                               bool(split_endpoints), dst.ptr, pitch,
                                                               torch.cuda.current_stream(src.device).cuda_stream))
    return out


# ---- BC7 -> RGBA8888 (include/dxtlt_bc7_image.h), BC6H -> RGBA16F (include/dxtlt_bc6h_image.h) ------------------------------
def _stream(device):
    import torch

    return torch.cuda.current_stream(device).cuda_stream


def _decode_granule_image(fmt, blocks, width, height, out, pitch):
    """``decode_bc7_image`` / ``decode_bc6h_image``: ``fmt`` is ``"bc7"`` / ``"bc6h"``"""
    from . import InvalidLength, _Buf

    src = _Buf(blocks, False)
    if src.device is None:
        raise TypeError(f"decode_{fmt}_image takes device tensors (the library has no host-pointer form of it)")
    if src.nbytes < image_blocks(width, height) * 16:
        raise InvalidLength(src.nbytes)
    out, dst, pitch = _output(src, width, height, out, pitch, _REGION_BPP[fmt])
    import torch

    with torch.cuda.device(src.device):
        _check(getattr(_l(), f"dxtlt_decode_{fmt}_image_device")(src.ptr, width, height, dst.ptr, pitch, _stream(src.device)))
    return out


def _untransform_decode_granule_image(fmt, transformed, width, height, first_block, total_blocks, out, pitch):
    """``untransform_decode_bc7_image`` / ``untransform_decode_bc6h_image``"""
    src, total_blocks = _whole_buffer(fmt, transformed, total_blocks)
    out, dst, pitch = _output(src, width, height, out, pitch, _REGION_BPP[fmt])
    call = f"dxtlt_untransform_decode_{fmt}_image"
    if src.device is None:
        _check(getattr(_l(), call)(src.ptr, total_blocks * 16, first_block, width, height, dst.ptr, pitch))
        return out
    import torch

    with torch.cuda.device(src.device):
        _check(getattr(_l(), call + "_device")(src.ptr, total_blocks, first_block, width, height, dst.ptr, pitch, _stream(src.device)))
    return out


def decode_bc7_image(blocks, width: int, height: int, out=None, pitch=None):
    """``blocks``: ceil(width / 4) * ceil(height / 4) BC7 blocks in block order, a CUDA tensor.  Returns ``out`` (a new tensor of
    ``pitch * height`` bytes when None); ``pitch`` defaults to ``4 * width``."""
    return _decode_granule_image("bc7", blocks, width, height, out, pitch)


def untransform_decode_bc7_image(transformed, width: int, height: int, *, first_block: int = 0, total_blocks=None, out=None, pitch=None):
    """``transformed``: the WHOLE buffer ``transform_bc7`` made, of ``total_blocks`` blocks (default: its length); the image is its
    blocks [first_block, first_block + ceil(width / 4) * ceil(height / 4)), ``first_block`` any block.  Returns ``out``."""
    return _untransform_decode_granule_image("bc7", transformed, width, height, first_block, total_blocks, out, pitch)


def decode_bc6h_image(blocks, width: int, height: int, out=None, pitch=None):
    """``blocks``: ceil(width / 4) * ceil(height / 4) BC6H (UF16) blocks in block order, a CUDA tensor.  Returns ``out`` (a new
    ``uint8`` tensor of ``pitch * height`` bytes when None); ``pitch`` defaults to ``8 * width``: a pixel is four half floats r, g, b,
    a with a = 1.0, and ``out.view(torch.float16).reshape(height, width, 4)`` is the image when the pitch is the default."""
    return _decode_granule_image("bc6h", blocks, width, height, out, pitch)


def untransform_decode_bc6h_image(transformed, width: int, height: int, *, first_block: int = 0, total_blocks=None, out=None, pitch=None):
    """``transformed``: the WHOLE buffer ``transform_bc6h`` made, of ``total_blocks`` blocks (default: its length); the image is its
    blocks [first_block, first_block + ceil(width / 4) * ceil(height / 4)), ``first_block`` any block.  Returns ``out``, ``uint8``;
    ``pitch`` defaults to ``8 * width``, and ``out.view(torch.float16).reshape(height, width, 4)`` is the image when the pitch is the
    default (``out.view(np.float16)`` for a host buffer)."""
    return _untransform_decode_granule_image("bc6h", transformed, width, height, first_block, total_blocks, out, pitch)


# ---- several images of one buffer ---------------------------------------------------------------------------------------
def mip_chain(width: int, height: int, mip_count: int, first_block: int = 0):
    """``([(first_block, level_width, level_height), ...], total_blocks)`` of a ``width`` x ``height`` chain of ``mip_count``
    levels whose level 0 starts at block ``first_block``; ``total_blocks`` is the block just behind the chain.  No device needed."""
    regions = (ImageRegion * max(1, mip_count))()
    total = C.c_uint64()
    _check(_l().dxtlt_image_mip_chain(width, height, mip_count, first_block, regions, C.byref(total)))
    return [(r.first_block, r.width, r.height) for r in regions[:mip_count]], total.value


def _region_table(fmt, src, regions, outs, pitches):
    """the outputs (new ones on the source's side where ``outs`` has none) and the DxtltImageRegion array"""
    regions = list(regions)
    outs = list(outs) if outs is not None else [None] * len(regions)
    pitches = list(pitches) if pitches is not None else [None] * len(regions)
    if len(outs) != len(regions) or len(pitches) != len(regions):
        raise ValueError("outs and pitches must have one entry per region")
    table, keep = (ImageRegion * max(1, len(regions)))(), []
    for i, (first, width, height) in enumerate(regions):
        outs[i], dst, pitch = _output(src, width, height, outs[i], pitches[i], _REGION_BPP[fmt])
        keep.append(dst)
        table[i] = ImageRegion(first, width, height, dst.ptr, pitch)
    return outs, table, len(regions), keep


def _whole_buffer(fmt, buffer, total_blocks):
    from . import InvalidLength, _Buf

    src, bs = _Buf(buffer, False), _REGION_BLOCK[fmt]
    if src.nbytes % bs != 0:
        raise InvalidLength(src.nbytes)
    if total_blocks is None:
        total_blocks = src.nbytes // bs
    if total_blocks * bs > src.nbytes:
        raise InvalidLength(src.nbytes)
    return src, total_blocks


def _symbol(fmt):
    """what a region call's name has between ``decode_`` and ``images``, and its leading format argument: BC7 and BC6H have entry
    points of their own"""
    return ("", (_ALL_FMT[fmt],)) if fmt in _ALL_FMT else (fmt + "_", ())


def _untransform_decode_regions(fmt, transformed, regions, total_blocks, outs, pitches, settings=()):
    """the fused region call of every format; ``settings``: the call's arguments behind the region list"""
    src, total_blocks = _whole_buffer(fmt, transformed, total_blocks)
    outs, table, count, keep = _region_table(fmt, src, regions, outs, pitches)
    symbol, head = _symbol(fmt)
    call = f"dxtlt_untransform_decode_{symbol}images"
    if src.device is None:
        _check(getattr(_l(), call)(*head, src.ptr, total_blocks * _REGION_BLOCK[fmt], table, count, *settings))
        return outs
    import torch

    with torch.cuda.device(src.device):
        _check(getattr(_l(), call + "_device")(*head, src.ptr, total_blocks, table, count, *settings, _stream(src.device)))
    del keep
    return outs


def _decode_regions(fmt, blocks, regions, total_blocks, outs, pitches):
    """the plain region call of every format"""
    src, total_blocks = _whole_buffer(fmt, blocks, total_blocks)
    symbol, head = _symbol(fmt)
    if src.device is None:
        raise TypeError(f"decode_{symbol}images takes device tensors (the library has no host-pointer form of it)")
    outs, table, count, keep = _region_table(fmt, src, regions, outs, pitches)
    import torch

    with torch.cuda.device(src.device):
        _check(getattr(_l(), f"dxtlt_decode_{symbol}images_device")(*head, src.ptr, total_blocks, table, count, _stream(src.device)))
    del keep
    return outs


def untransform_decode_images(fmt: str, transformed, regions, *, total_blocks=None, decorrelation_mode=0,
                              split_alpha_endpoints: bool = False, split_colour_endpoints: bool = False, split_endpoints=None,
                              outs=None, pitches=None):
    """Every region ``(first_block, width, height)`` of the WHOLE transformed buffer ``transformed`` (``total_blocks`` blocks,
    default: its length) to an image of its own, in one call: one or two launches per sixteen regions.  ``fmt`` is ``"bc1"`` ..
    ``"bc5"``; ``"bc4"`` / ``"bc5"`` take ``split_endpoints`` (or ``split_alpha_endpoints``, as the C call does) and ignore the
    other settings.  The regions ascend and do not overlap.  Returns the list of outputs: ``outs[i]``, or a new buffer of
    ``pitch * height`` bytes where it is None; ``pitches[i]`` defaults to ``bpp * width``."""
    if fmt in _CHANNEL_FMT and split_endpoints is not None:
        split_alpha_endpoints = split_endpoints
    settings = (int(decorrelation_mode), bool(split_alpha_endpoints), bool(split_colour_endpoints))
    return _untransform_decode_regions(fmt, transformed, regions, total_blocks, outs, pitches, settings)


def decode_images(fmt: str, blocks, regions, *, total_blocks=None, outs=None, pitches=None):
    """The same from a block array in block order, a CUDA tensor (the library has no host-pointer form of it)."""
    return _decode_regions(fmt, blocks, regions, total_blocks, outs, pitches)


def untransform_decode_bc7_images(transformed, regions, *, total_blocks=None, outs=None, pitches=None):
    """``untransform_decode_images`` for BC7 (include/dxtlt_bc7_image.h): every region ``(first_block, width, height)`` of the
    WHOLE buffer ``transform_bc7`` made to an RGBA8888 image of its own, every granule un-sorted and decoded once.  Regions as
    ``mip_chain`` returns them; host buffers or CUDA tensors (torch's current stream).  Returns the list of outputs."""
    return _untransform_decode_regions("bc7", transformed, regions, total_blocks, outs, pitches)


def decode_bc7_images(blocks, regions, *, total_blocks=None, outs=None, pitches=None):
    """The same from a BC7 block array in block order, a CUDA tensor (the library has no host-pointer form of it)."""
    return _decode_regions("bc7", blocks, regions, total_blocks, outs, pitches)


def untransform_decode_bc6h_images(transformed, regions, *, total_blocks=None, outs=None, pitches=None):
    """``untransform_decode_images`` for BC6H (include/dxtlt_bc6h_image.h): every region ``(first_block, width, height)`` of the
    WHOLE buffer ``transform_bc6h`` made to an RGBA16F image of its own, every granule un-sorted and decoded once.  Regions as
    ``mip_chain`` returns them; host buffers or CUDA tensors (torch's current stream).  Returns the list of outputs, ``uint8``;
    ``pitches[i]`` defaults to ``8 * width``, and ``out.view(torch.float16).reshape(height, width, 4)`` is the image then."""
    return _untransform_decode_regions("bc6h", transformed, regions, total_blocks, outs, pitches)


def decode_bc6h_images(blocks, regions, *, total_blocks=None, outs=None, pitches=None):
    """The same from a BC6H block array in block order, a CUDA tensor (the library has no host-pointer form of it)."""
    return _decode_regions("bc6h", blocks, regions, total_blocks, outs, pitches)


# ---- many buffers in one call -------------------------------------------------------------------------------------------
def untransform_decode_images_batch(items):
    """The images of many transformed buffers in ONE call: one launch per (format, settings) present in ``items``.

    An item is ``(fmt, transformed, regions)`` or ``(fmt, transformed, regions, settings)``, ``settings`` a dict of the
    keyword arguments of ``untransform_decode_images`` (``total_blocks``, ``decorrelation_mode``, ``split_alpha_endpoints``,
    ``split_colour_endpoints``, ``split_endpoints``, ``outs``, ``pitches``).  Every ``transformed`` is a CUDA ``torch.uint8``
    tensor, all on one device; the call is enqueued on torch's current stream of that device.  Returns one list of outputs per
    item, as ``untransform_decode_images`` returns them.  Items may mix formats, settings and sizes; the images must not
    overlap."""
    import torch

    items = list(items)
    table, keep, results, device = (ImageBatchItem * max(1, len(items)))(), [], [], None
    for k, item in enumerate(items):
        fmt, transformed, regions = item[0], item[1], item[2]
        kw = dict(item[3]) if len(item) > 3 and item[3] is not None else {}
        src, total_blocks = _whole_buffer(fmt, transformed, kw.pop("total_blocks", None))
        if src.device is None:
            raise TypeError("untransform_decode_images_batch takes device tensors (the library has no host-pointer form of it)")
        if device is None:
            device = src.device
        if src.device != device:
            raise TypeError("all buffers of a batch must be tensors on one device")
        outs, regions_c, count, dsts = _region_table(fmt, src, regions, kw.pop("outs", None), kw.pop("pitches", None))
        sa = kw.pop("split_alpha_endpoints", False)
        split_endpoints = kw.pop("split_endpoints", None)
        if fmt in _CHANNEL_FMT and split_endpoints is not None:
            sa = split_endpoints
        mode, sc = int(kw.pop("decorrelation_mode", 0)), bool(kw.pop("split_colour_endpoints", False))
        if kw:
            raise TypeError(f"unknown settings of batch item {k}: {sorted(kw)}")
        table[k] = ImageBatchItem(src.ptr, total_blocks, C.cast(regions_c, C.c_void_p), count, _ALL_FMT[fmt], mode, int(bool(sa)), int(sc))
        keep.append((src, regions_c, dsts))
        results.append(outs)
    if not items:
        return results
    with torch.cuda.device(device):
        _check(_l().dxtlt_untransform_decode_images_batch_device(table, len(items), torch.cuda.current_stream(device).cuda_stream))
    del keep
    return results


def _untransform_decode_granule_images_batch(fmt, item_type, entry, items):
    """``untransform_decode_bc7_images_batch`` / ``untransform_decode_bc6h_images_batch``: ``fmt`` is ``"bc7"`` / ``"bc6h"``"""
    import torch

    items = list(items)
    table, keep, results, device = (item_type * max(1, len(items)))(), [], [], None
    for k, item in enumerate(items):
        transformed, regions = item[0], item[1]
        kw = dict(item[2]) if len(item) > 2 and item[2] is not None else {}
        src, total_blocks = _whole_buffer(fmt, transformed, kw.pop("total_blocks", None))
        if src.device is None:
            raise TypeError(f"untransform_decode_{fmt}_images_batch takes device tensors (the library has no host-pointer form of it)")
        if device is None:
            device = src.device
        if src.device != device:
            raise TypeError("all buffers of a batch must be tensors on one device")
        outs, regions_c, count, dsts = _region_table(fmt, src, regions, kw.pop("outs", None), kw.pop("pitches", None))
        if kw:
            raise TypeError(f"unknown options of batch item {k}: {sorted(kw)}")
        table[k] = item_type(src.ptr, total_blocks, C.cast(regions_c, C.c_void_p), count, 0)
        keep.append((src, regions_c, dsts))
        results.append(outs)
    if not items:
        return results
    with torch.cuda.device(device):
        _check(getattr(_l(), entry)(table, len(items), torch.cuda.current_stream(device).cuda_stream))
    del keep
    return results


def untransform_decode_bc7_images_batch(items):
    """The images of many BC7 transformed buffers in ONE call (include/dxtlt_bc7_image.h): at most two launches, whatever the
    number of buffers.

    An item is ``(transformed, regions)`` or ``(transformed, regions, opts)``, ``opts`` a dict of ``total_blocks``, ``outs`` and
    ``pitches`` as ``untransform_decode_bc7_images`` takes them.  Every ``transformed`` is a CUDA ``torch.uint8`` tensor, all on
    one device; the call is enqueued on torch's current stream of that device.  Returns one list of outputs per item, as
    ``untransform_decode_bc7_images`` returns them.  Items may differ in size and region layout; the images must not overlap."""
    return _untransform_decode_granule_images_batch("bc7", Bc7ImageBatchItem, "dxtlt_untransform_decode_bc7_images_batch_device", items)


def untransform_decode_bc6h_images_batch(items):
    """The images of many BC6H transformed buffers in ONE call (include/dxtlt_bc6h_image.h): at most two launches, whatever the
    number of buffers.

    Items, options, conventions and errors are those of ``untransform_decode_bc7_images_batch``; the buffers are the ones
    ``transform_bc6h`` made, the outputs ``uint8`` tensors of RGBA16F pixels, the default pitch ``8 * width``, as
    ``untransform_decode_bc6h_images`` returns them."""
    return _untransform_decode_granule_images_batch("bc6h", Bc6hImageBatchItem, "dxtlt_untransform_decode_bc6h_images_batch_device", items)
