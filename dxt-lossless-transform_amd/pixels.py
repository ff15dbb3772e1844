"""Uncompressed pixels -- RGBA8888 / BGRA8888 (4 bytes per pixel) and BGR888 (3) -- in this build's layout, version 1
(docs/PIXEL_FORMAT.md); upstream has no transform for them.  Thin Python layer over include/dxtlt_pixels.h, the same buffer
conventions as bc6h.py: host buffers (numpy uint8 / bytes / bytearray) or CUDA uint8 tensors on torch's current stream."""
from __future__ import annotations

import ctypes as C

from . import _lib

INTERLEAVED, PLANAR, PLANAR_DELTA = 0, 1, 2
SEGMENT = 4096

_declared = False


def _l():
    global _declared
    l = _lib.load()
    if not _declared:
        vp, sz, i32, b, u8, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_bool, C.c_uint8, C.c_uint64
        for n in ("dxtlt_transform_pixels", "dxtlt_untransform_pixels"):
            getattr(l, n).argtypes, getattr(l, n).restype = [vp, vp, sz, i32, b, u8], i32
        for n in ("dxtlt_transform_pixels_device", "dxtlt_untransform_pixels_device"):
            getattr(l, n).argtypes, getattr(l, n).restype = [vp, vp, sz, i32, b, u8, vp], i32
        l.dxtlt_transform_pixels_range_device.argtypes = [i32, b, vp, vp, u64, u64, u64, b, u8, vp]
        l.dxtlt_transform_pixels_range_device.restype = i32
        _declared = True
    return l


def _check_settings(pixel_bytes: int, layout: int) -> None:
    if pixel_bytes not in (3, 4):
        raise ValueError("pixel_bytes must be 4 (RGBA8888, BGRA8888) or 3 (BGR888)")
    if layout not in (INTERLEAVED, PLANAR, PLANAR_DELTA):
        raise ValueError("layout must be INTERLEAVED, PLANAR or PLANAR_DELTA")


def _run(inverse: bool, input, output, pixel_bytes: int, decorrelate: bool, layout: int) -> None:
    from . import DeviceError, InvalidLength, OutputBufferTooSmall, _Buf

    _check_settings(pixel_bytes, layout)
    src, dst = _Buf(input, False), _Buf(output, True)
    if src.nbytes % pixel_bytes != 0:
        raise InvalidLength(src.nbytes)
    if dst.nbytes < src.nbytes:
        raise OutputBufferTooSmall(src.nbytes, dst.nbytes)
    if (src.device is None) != (dst.device is None):
        raise TypeError("input and output must both be host buffers or both be device tensors")
    l = _l()
    name = "dxtlt_untransform_pixels" if inverse else "dxtlt_transform_pixels"
    if src.device is None:
        rc = getattr(l, name)(src.ptr, dst.ptr, src.nbytes, pixel_bytes, bool(decorrelate), layout)
    else:
        import torch

        with torch.cuda.device(src.device):
            stream = torch.cuda.current_stream().cuda_stream
            rc = getattr(l, name + "_device")(src.ptr, dst.ptr, src.nbytes, pixel_bytes, bool(decorrelate), layout, stream)
    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())


def transform_pixels(input, output, pixel_bytes: int = 4, decorrelate: bool = True, layout: int = PLANAR_DELTA) -> None:
    _run(False, input, output, pixel_bytes, decorrelate, layout)


def untransform_pixels(input, output, pixel_bytes: int = 4, decorrelate: bool = True, layout: int = PLANAR_DELTA) -> None:
    _run(True, input, output, pixel_bytes, decorrelate, layout)


def transform_pixels_range(inverse: bool, src, dst, total_pixels: int, first_pixel: int, num_pixels: int, pixel_bytes: int = 4,
                           decorrelate: bool = True, layout: int = PLANAR_DELTA) -> None:
    """dxtlt_transform_pixels_range_device on torch CUDA tensors: the interleaved-side tensor starts at pixel `first_pixel` (a
    multiple of SEGMENT), the transformed-side tensor is the whole transformed buffer."""
    import torch

    from . import DeviceError, OutputBufferTooSmall, _Buf

    _check_settings(pixel_bytes, layout)
    s, d = _Buf(src, False), _Buf(dst, True)
    if s.device is None or d.device is None:
        raise TypeError("transform_pixels_range takes device tensors")
    inter, trans = (d, s) if inverse else (s, d)
    if inter.nbytes < num_pixels * pixel_bytes or trans.nbytes < total_pixels * pixel_bytes:
        raise OutputBufferTooSmall(max(num_pixels, total_pixels) * pixel_bytes, min(inter.nbytes, trans.nbytes))
    with torch.cuda.device(s.device):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _l().dxtlt_transform_pixels_range_device(pixel_bytes, bool(inverse), s.ptr, d.ptr, total_pixels, first_pixel, num_pixels,
                                                      bool(decorrelate), layout, stream)
    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())


# the candidates of transform_auto as (decorrelate, layout), in the order they are compared; ties keep the earlier one
AUTO_CANDIDATES = [(True, PLANAR_DELTA), (True, PLANAR), (True, INTERLEAVED), (False, PLANAR_DELTA), (False, PLANAR), (False, INTERLEAVED)]


def transform_auto(input, output, pixel_bytes: int = 4, estimator=None):
    """The pixel auto transform (dxtlt_transform_pixels_auto / _auto_device): the best of the six settings by the entropy
    estimator, chosen on the device.  Host buffers or CUDA uint8 tensors (torch's current stream: waited for once, the winner's
    transform left enqueued).  `estimator`: a pointer to a DltSizeEstimator for host buffers (default: the entropy estimator,
    everything on the device; any other is called per candidate).  Returns (decorrelate, layout); `output` holds the data
    transformed with them."""
    from . import DeviceError, InvalidLength, OutputBufferTooSmall, _Buf
    from . import estimator as _estimator

    if pixel_bytes not in (3, 4):
        raise ValueError("pixel_bytes must be 4 (RGBA8888, BGRA8888) or 3 (BGR888)")
    src, dst = _Buf(input, False), _Buf(output, True)
    if src.nbytes % pixel_bytes != 0:
        raise InvalidLength(src.nbytes)
    if dst.nbytes < src.nbytes:
        raise OutputBufferTooSmall(src.nbytes, dst.nbytes)
    if (src.device is None) != (dst.device is None):
        raise TypeError("input and output must both be host buffers or both be device tensors")
    l = _estimator._l()
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
    dec, lay = C.c_bool(), C.c_uint8()
    if src.device is None:
        est = estimator if estimator is not None else _estimator.builtin_entropy_estimator()
        f = l.dxtlt_transform_pixels_auto
        f.argtypes, f.restype = [vp, vp, sz, i32, vp, C.POINTER(C.c_bool), C.POINTER(C.c_uint8)], i32
        rc = f(src.ptr, dst.ptr, src.nbytes, pixel_bytes, C.cast(est, vp), C.byref(dec), C.byref(lay))
    else:
        import torch

        if estimator is not None:
            raise TypeError("device tensors are ranked by the entropy estimator; an estimator of the caller's takes host buffers")
        f = l.dxtlt_transform_pixels_auto_device
        f.argtypes, f.restype = [vp, vp, sz, i32, vp, C.POINTER(C.c_bool), C.POINTER(C.c_uint8)], i32
        with torch.cuda.device(src.device):
            rc = f(src.ptr, dst.ptr, src.nbytes, pixel_bytes, torch.cuda.current_stream().cuda_stream, C.byref(dec), C.byref(lay))
    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())
    return bool(dec.value), int(lay.value)


def last_auto_totals():
    """The six totals the last transform_auto of this thread compared, in the order of AUTO_CANDIDATES ([] after a call with an
    estimator of the caller's, an empty buffer or a failed call)."""
    from . import estimator as _estimator

    l = _estimator._l()
    l.dxtlt_debug_pixels_auto_last_totals.argtypes, l.dxtlt_debug_pixels_auto_last_totals.restype = [C.POINTER(C.c_uint64), C.c_int32], C.c_int32
    buf = (C.c_uint64 * 6)()
    n = l.dxtlt_debug_pixels_auto_last_totals(buf, 6)
    return [int(v) for v in buf[:n]]


class PixelBatchItem(C.Structure):               # DxtltPixelBatchItem
    _fields_ = [("d_input", C.c_void_p), ("d_output", C.c_void_p), ("len", C.c_uint64), ("pixel_bytes", C.c_uint8),
                ("inverse", C.c_uint8), ("decorrelate", C.c_uint8), ("layout", C.c_uint8), ("reserved", C.c_uint8 * 4)]


class PixelBatchAutoItem(C.Structure):           # DxtltPixelBatchAutoItem
    _fields_ = [("d_input", C.c_void_p), ("d_output", C.c_void_p), ("len", C.c_uint64), ("pixel_bytes", C.c_uint8),
                ("decorrelate", C.c_uint8), ("layout", C.c_uint8), ("reserved", C.c_uint8 * 5)]


def _batch_buffers(name: str, k: int, src, dst, pixel_bytes: int, device):
    """the two tensors of item `k` as (_Buf, _Buf, device), checked as the single calls check them"""
    from . import InvalidLength, OutputBufferTooSmall, _Buf

    s, d = _Buf(src, False), _Buf(dst, True)
    if s.device is None or d.device is None:
        raise TypeError(name + " takes device tensors")
    device = s.device if device is None else device
    if s.device != device or d.device != device:
        raise ValueError("all tensors of a batch must live on one device")
    if pixel_bytes not in (3, 4):
        raise ValueError("pixel_bytes must be 4 (RGBA8888, BGRA8888) or 3 (BGR888)")
    if s.nbytes % pixel_bytes != 0:
        raise InvalidLength(s.nbytes)
    if d.nbytes < s.nbytes:
        raise OutputBufferTooSmall(s.nbytes, d.nbytes)
    return s, d, device


def _stream_of(stream):
    import torch

    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def transform_pixels_batch(items, stream=None) -> None:
    """dxtlt_transform_pixels_batch_device: items are (input tensor, output tensor, pixel_bytes, inverse, decorrelate, layout) with
    CUDA uint8 tensors on one device.  Every item is transformed (inverse false) or untransformed exactly as the single calls do
    it, with one launch per (pixel_bytes, inverse, decorrelate, layout) class present: enqueued on `stream` (a torch stream or a
    raw handle; default torch's current stream), not waited for.  An output may overlap no other buffer of the batch."""
    import torch

    from . import DeviceError

    if not items:
        return
    arr = (PixelBatchItem * len(items))()
    device, keep = None, []
    for k, (src, dst, pixel_bytes, inverse, decorrelate, layout) in enumerate(items):
        _check_settings(pixel_bytes, layout)
        s, d, device = _batch_buffers("transform_pixels_batch", k, src, dst, pixel_bytes, device)
        arr[k].d_input, arr[k].d_output, arr[k].len = s.ptr, d.ptr, s.nbytes
        arr[k].pixel_bytes, arr[k].inverse, arr[k].decorrelate, arr[k].layout = pixel_bytes, int(bool(inverse)), int(bool(decorrelate)), layout
        keep.append((s, d))
    l = _l()
    l.dxtlt_transform_pixels_batch_device.argtypes = [C.POINTER(PixelBatchItem), C.c_size_t, C.c_void_p]
    l.dxtlt_transform_pixels_batch_device.restype = C.c_int32
    with torch.cuda.device(device):
        rc = l.dxtlt_transform_pixels_batch_device(arr, len(arr), _stream_of(stream))
    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())


def transform_batch_auto(items, stream=None):
    """dxtlt_transform_pixels_batch_auto_device: items are (input tensor, output tensor, pixel_bytes) with CUDA uint8 tensors on
    one device.  Chooses the best of the six settings for every item with the entropy estimator and transforms them all on `stream`
    (default torch's current stream): one stream wait and a launch count that does not grow with the number of items.  Returns
    the list of (decorrelate, layout), one per item; the transforms are enqueued, not waited for."""
    import torch

    from . import DeviceError

    if not items:
        return []
    arr = (PixelBatchAutoItem * len(items))()
    device, keep = None, []
    for k, (src, dst, pixel_bytes) in enumerate(items):
        s, d, device = _batch_buffers("transform_batch_auto", k, src, dst, pixel_bytes, device)
        arr[k].d_input, arr[k].d_output, arr[k].len, arr[k].pixel_bytes = s.ptr, d.ptr, s.nbytes, pixel_bytes
        keep.append((s, d))
    l = _l()
    l.dxtlt_transform_pixels_batch_auto_device.argtypes = [C.POINTER(PixelBatchAutoItem), C.c_size_t, C.c_void_p]
    l.dxtlt_transform_pixels_batch_auto_device.restype = C.c_int32
    with torch.cuda.device(device):
        rc = l.dxtlt_transform_pixels_batch_auto_device(arr, len(arr), _stream_of(stream))
    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())
    return [(bool(a.decorrelate), int(a.layout)) for a in arr]


def last_batch_auto_totals(item: int):
    """The six totals the last transform_batch_auto of this thread compared for item `item`, in the order of AUTO_CANDIDATES ([]
    for an empty item, an item out of range or a failed call)."""
    l = _l()
    f = l.dxtlt_debug_pixels_batch_auto_last_totals
    f.argtypes, f.restype = [C.c_size_t, C.POINTER(C.c_uint64), C.c_int32], C.c_int32
    buf = (C.c_uint64 * 6)()
    n = f(int(item), buf, 6)
    return [int(v) for v in buf[:n]]


def debug_auto_candidates_into(input, arena, pixel_bytes: int = 4) -> None:
    """Test hook (dxtlt_debug_pixels_auto_candidates_into_device): the fused candidate kernel of transform_auto from the CUDA uint8
    tensor `input` (on a 16-byte boundary) into the caller's `arena` of 5 * len bytes or more -- candidate i of AUTO_CANDIDATES[:5]
    at arena[i * len:(i + 1) * len].  Enqueued on torch's current stream, not waited for."""
    import torch

    from . import DeviceError, OutputBufferTooSmall, _Buf

    src, dst = _Buf(input, False), _Buf(arena, True)
    if src.device is None or dst.device is None:
        raise TypeError("debug_auto_candidates_into takes device tensors")
    if dst.nbytes < 5 * src.nbytes:
        raise OutputBufferTooSmall(5 * src.nbytes, dst.nbytes)
    f = _l().dxtlt_debug_pixels_auto_candidates_into_device
    f.argtypes, f.restype = [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p], C.c_int32
    with torch.cuda.device(src.device):
        rc = f(src.ptr, src.nbytes, pixel_bytes, dst.ptr, torch.cuda.current_stream().cuda_stream)
    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())


def debug_batch_candidates(items, chunk: int, arena, stream=None) -> None:
    """Test hook (dxtlt_debug_pixels_batch_candidates_device): the candidate launches of chunk `chunk` of transform_batch_auto over
    `items` -- (input tensor, output tensor, pixel_bytes), as there; no output is written -- into the caller's CUDA uint8 tensor
    `arena`: item k's five candidates at the arena_offset dxtlt_debug_plan_pixels_batch_auto reports for it.  Waits for `stream`."""
    import torch

    from . import DeviceError, _Buf

    arr = (PixelBatchAutoItem * max(1, len(items)))()
    device, keep = None, []
    for k, (src, dst, pixel_bytes) in enumerate(items):
        s, d, device = _batch_buffers("debug_batch_candidates", k, src, dst, pixel_bytes, device)
        arr[k].d_input, arr[k].d_output, arr[k].len, arr[k].pixel_bytes = s.ptr, d.ptr, s.nbytes, pixel_bytes
        keep.append((s, d))
    a = _Buf(arena, True)
    if a.device is None:
        raise TypeError("debug_batch_candidates takes a device tensor as its arena")
    f = _l().dxtlt_debug_pixels_batch_candidates_device
    f.argtypes = [C.POINTER(PixelBatchAutoItem), C.c_size_t, C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p]
    f.restype = C.c_int32
    with torch.cuda.device(a.device):
        rc = f(arr, len(items), int(chunk), a.ptr, a.nbytes, _stream_of(stream))
    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())


def settings_triple(decorrelate: bool, layout: int):
    """(decorrelation_mode, split_alpha_endpoints, split_colour_endpoints) as the generic entry points -- the host batch call's
    format codes 8 / 9, dxtlt_transform_sharded, the DDS calls -- read these settings"""
    return (1 if decorrelate else 0), layout == PLANAR_DELTA, layout != INTERLEAVED


def transform_pixels_sharded(input, output, pixel_bytes: int = 4, decorrelate: bool = True, layout: int = PLANAR_DELTA,
                             num_shards: int = 0, inverse: bool = False) -> None:
    """Host buffers, pixel range sharded on segments over the node's GPUs inside this process (dxtlt_transform_sharded with
    format code 8 / 9).  ``num_shards`` <= 0: one shard per device; more shards than devices run round robin."""
    from . import DeviceError, InvalidLength, OutputBufferTooSmall, _Buf

    _check_settings(pixel_bytes, layout)
    src, dst = _Buf(input, False), _Buf(output, True)
    if src.device is not None or dst.device is not None:
        raise TypeError("transform_pixels_sharded takes host buffers")
    if src.nbytes % pixel_bytes != 0:
        raise InvalidLength(src.nbytes)
    if dst.nbytes < src.nbytes:
        raise OutputBufferTooSmall(src.nbytes, dst.nbytes)
    mode, sa, sc = settings_triple(decorrelate, layout)
    rc = _l().dxtlt_transform_sharded(8 if pixel_bytes == 4 else 9, bool(inverse), src.ptr, dst.ptr, src.nbytes, mode, sa, sc,
                                      int(num_shards))
    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())
