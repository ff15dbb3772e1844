"""The built-in, device-resident size estimator (docs/ESTIMATOR.md, version 1) and the auto transforms that use it without
moving a section over PCIe.  Thin ctypes layer over include/dxtlt_estimator.h, the same buffer conventions as bc6h.py: host
buffers (bytes, numpy) or contiguous uint8 torch CUDA tensors."""
from __future__ import annotations

import ctypes as C

from . import _lib

MAXFN = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))
ESTFN = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))


class DltSizeEstimator(C.Structure):            # include/dlt_size_estimator.h
    _fields_ = [("Context", C.c_void_p), ("MaxCompressedSize", MAXFN), ("EstimateCompressedSize", ESTFN)]


class Section(C.Structure):                     # DxtltEstimateSection
    _fields_ = [("d_ptr", C.c_void_p), ("len", C.c_uint64)]


class BatchAutoItem(C.Structure):               # DxtltBatchAutoItem
    _fields_ = [("d_input", C.c_void_p), ("d_output", C.c_void_p), ("len", C.c_uint64), ("format", C.c_uint8),
                ("use_all_decorrelation_modes", C.c_uint8), ("decorrelation_mode", C.c_uint8),
                ("split_alpha_endpoints", C.c_uint8), ("split_colour_endpoints", C.c_uint8), ("reserved", C.c_uint8 * 3)]


_own = None


def _l():
    """A ctypes handle of this module's own on the loaded library: the argument types declared here (the host-pointer auto calls
    among them) are not shared with other declarations of the same symbols."""
    global _own
    if _own is None:
        _lib.load()
        l = C.CDLL(_lib.lib_path(), mode=C.RTLD_GLOBAL)
        vp, sz, i32, b = C.c_void_p, C.c_size_t, C.c_int32, C.c_bool
        u8p, bp, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_bool), C.POINTER(C.c_uint64)
        l.dxtlt_estimator_version.argtypes, l.dxtlt_estimator_version.restype = [], C.c_uint32
        l.dxtlt_estimate_sizes_device.argtypes, l.dxtlt_estimate_sizes_device.restype = [C.POINTER(Section), sz, vp, vp], i32
        l.dxtlt_estimate_size_device.argtypes, l.dxtlt_estimate_size_device.restype = [vp, sz, vp, u64p], i32
        l.dxtlt_estimate_size.argtypes, l.dxtlt_estimate_size.restype = [vp, sz, u64p], i32
        l.dxtlt_builtin_size_estimator.argtypes, l.dxtlt_builtin_size_estimator.restype = [], C.POINTER(DltSizeEstimator)
        for n in ("bc1", "bc2"):
            f = getattr(l, f"dxtlt_transform_{n}_auto_device")
            f.argtypes, f.restype = [vp, vp, sz, b, vp, u8p, bp], i32
            f = getattr(l, f"dxtlt_transform_{n}_auto")
            f.argtypes, f.restype = [vp, vp, sz, C.POINTER(DltSizeEstimator), b, u8p, bp, C.POINTER(C.c_uint32)], i32
        l.dxtlt_transform_bc3_auto_device.argtypes, l.dxtlt_transform_bc3_auto_device.restype = [vp, vp, sz, b, vp, u8p, bp, bp], i32
        l.dxtlt_transform_bc3_auto.argtypes = [vp, vp, sz, C.POINTER(DltSizeEstimator), b, u8p, bp, bp, C.POINTER(C.c_uint32)]
        l.dxtlt_transform_bc3_auto.restype = i32
        for n in ("bc4", "bc5"):
            f = getattr(l, f"dxtlt_transform_{n}_auto_device")
            f.argtypes, f.restype = [vp, vp, sz, b, vp, bp], i32
            f = getattr(l, f"dxtlt_transform_{n}_auto")
            f.argtypes, f.restype = [vp, vp, sz, C.POINTER(DltSizeEstimator), bp], i32
        l.dxtlt_debug_auto_last_estimation.argtypes, l.dxtlt_debug_auto_last_estimation.restype = [u64p, u64p], None
        l.dxtlt_debug_auto_last_totals.argtypes, l.dxtlt_debug_auto_last_totals.restype = [u64p, i32], i32
        l.dxtlt_debug_auto_use_arena.argtypes, l.dxtlt_debug_auto_use_arena.restype = [i32], None
        l.dxtlt_debug_estimate_sizes_shape.argtypes = [C.POINTER(Section), sz, vp, vp, i32, C.c_uint32, C.c_uint32]
        l.dxtlt_debug_estimate_sizes_shape.restype = i32
        l.dxtlt_debug_auto_candidates_device.argtypes, l.dxtlt_debug_auto_candidates_device.restype = [i32, b, vp, sz, vp], i32
        l.dxtlt_transform_batch_auto_device.argtypes = [C.POINTER(BatchAutoItem), sz, vp]
        l.dxtlt_transform_batch_auto_device.restype = i32
        l.dxtlt_debug_batch_auto_last.argtypes, l.dxtlt_debug_batch_auto_last.restype = [u64p], None
        l.dxtlt_debug_batch_auto_last_totals.argtypes, l.dxtlt_debug_batch_auto_last_totals.restype = [sz, u64p, i32], i32
        l.dxtlt_debug_batch_auto_arena_cap.argtypes, l.dxtlt_debug_batch_auto_arena_cap.restype = [C.c_uint64], None
        l.dxtlt_debug_batch_auto_time_phases.argtypes, l.dxtlt_debug_batch_auto_time_phases.restype = [i32], None
        l.dxtlt_debug_batch_auto_last_phase_ms.argtypes, l.dxtlt_debug_batch_auto_last_phase_ms.restype = [C.POINTER(C.c_double)], None
        # the entropy estimator (include/dxtlt_entropy_estimator.h)
        l.dxtlt_entropy_estimator_version.argtypes, l.dxtlt_entropy_estimator_version.restype = [], C.c_uint32
        l.dxtlt_estimate_entropy_sizes_device.argtypes = [C.POINTER(Section), sz, vp, vp]
        l.dxtlt_estimate_entropy_sizes_device.restype = i32
        l.dxtlt_estimate_entropy_size_device.argtypes, l.dxtlt_estimate_entropy_size_device.restype = [vp, sz, vp, u64p], i32
        l.dxtlt_estimate_entropy_size.argtypes, l.dxtlt_estimate_entropy_size.restype = [vp, sz, u64p], i32
        l.dxtlt_builtin_entropy_estimator.argtypes, l.dxtlt_builtin_entropy_estimator.restype = [], C.POINTER(DltSizeEstimator)
        l.dxtlt_debug_entropy_table.argtypes, l.dxtlt_debug_entropy_table.restype = [C.c_uint32], C.c_uint32
        _own = l
    return _own


def _check(rc: int) -> None:
    from . import DeviceError

    if rc != _lib.OK:
        raise DeviceError(rc, _lib.last_error())


def version() -> int:
    return int(_l().dxtlt_estimator_version())


def builtin_size_estimator():
    """Pointer to the process-lifetime DltSizeEstimator; hand it to any *_auto entry point."""
    return _l().dxtlt_builtin_size_estimator()


def estimate_size(data) -> int:
    """The estimate of one section: a host buffer (uploaded) or a device tensor (current stream; waits for it)."""
    from . import _Buf

    src = _Buf(data, False)
    out = C.c_uint64()
    l = _l()
    if src.device is None:
        _check(l.dxtlt_estimate_size(src.ptr, src.nbytes, C.byref(out)))
    else:
        import torch

        with torch.cuda.device(src.device):
            _check(l.dxtlt_estimate_size_device(src.ptr, src.nbytes, torch.cuda.current_stream().cuda_stream, C.byref(out)))
    return int(out.value)


def entropy_version() -> int:
    """The version of the entropy estimator (docs/ESTIMATOR.md, "The entropy estimator, version 1")."""
    return int(_l().dxtlt_entropy_estimator_version())


def builtin_entropy_estimator():
    """Pointer to the process-lifetime DltSizeEstimator of the entropy estimator; what pixels.transform_auto uses."""
    return _l().dxtlt_builtin_entropy_estimator()


def entropy_table(k: int) -> int:
    """T[k] = floor(2^16 log2 k) as the kernels read it (host side, no device)."""
    return int(_l().dxtlt_debug_entropy_table(int(k)))


def estimate_entropy_size(data) -> int:
    """The entropy estimate of one section: a host buffer (uploaded) or a device tensor (current stream; waits for it)."""
    from . import _Buf

    src = _Buf(data, False)
    out = C.c_uint64()
    l = _l()
    if src.device is None:
        _check(l.dxtlt_estimate_entropy_size(src.ptr, src.nbytes, C.byref(out)))
    else:
        import torch

        with torch.cuda.device(src.device):
            _check(l.dxtlt_estimate_entropy_size_device(src.ptr, src.nbytes, torch.cuda.current_stream().cuda_stream, C.byref(out)))
    return int(out.value)


def estimate_entropy_sizes(sections, out) -> None:
    """dxtlt_estimate_entropy_sizes_device: `sections` are device tensors, `out` an int64 / uint64 device tensor of as many
    elements.  Enqueues on the current stream and returns; nothing is synchronised."""
    import torch

    from . import _Buf

    bufs = [_Buf(s, False) for s in sections]
    if any(b.device is None for b in bufs) or not out.is_cuda:
        raise TypeError("estimate_entropy_sizes takes device tensors")
    if out.element_size() != 8 or out.numel() < len(bufs) or not out.is_contiguous():
        raise TypeError("out must be a contiguous 8-byte integer tensor with one element per section")
    table = (Section * max(1, len(bufs)))()
    for t, b in zip(table, bufs):
        t.d_ptr, t.len = b.ptr, b.nbytes
    with torch.cuda.device(out.device):
        _check(_l().dxtlt_estimate_entropy_sizes_device(table, len(bufs), torch.cuda.current_stream().cuda_stream, out.data_ptr()))


def estimate_sizes(sections, out, shape=None) -> None:
    """dxtlt_estimate_sizes_device: `sections` are device tensors, `out` an int64 / uint64 device tensor of as many elements.
    Enqueues on the current stream and returns; nothing is synchronised.  `shape` = (lanes, window, bits) goes through the
    test / bench hook dxtlt_debug_estimate_sizes_shape instead."""
    import torch

    from . import _Buf

    bufs = [_Buf(s, False) for s in sections]
    if any(b.device is None for b in bufs) or not out.is_cuda:
        raise TypeError("estimate_sizes takes device tensors")
    if out.element_size() != 8 or out.numel() < len(bufs) or not out.is_contiguous():
        raise TypeError("out must be a contiguous 8-byte integer tensor with one element per section")
    table = (Section * max(1, len(bufs)))()
    for t, b in zip(table, bufs):
        t.d_ptr, t.len = b.ptr, b.nbytes
    with torch.cuda.device(out.device):
        stream = torch.cuda.current_stream().cuda_stream
        if shape is None:
            _check(_l().dxtlt_estimate_sizes_device(table, len(bufs), stream, out.data_ptr()))
        else:
            _check(_l().dxtlt_debug_estimate_sizes_shape(table, len(bufs), stream, out.data_ptr(), *[int(v) for v in shape]))


def transform_auto(fmt: str, input, output, use_all_decorrelation_modes: bool = False):
    """transform_bcN_auto with the built-in estimator, fmt in bc1..bc5, on host buffers or device tensors.  Returns the
    chosen settings object (Bc1TransformSettings ...); `output` holds the data transformed with them."""
    from . import (BLOCK_BYTES, Bc1TransformSettings, Bc2TransformSettings, Bc3TransformSettings, Bc4TransformSettings,
                   Bc5TransformSettings, InvalidLength, OutputBufferTooSmall, YCoCgVariant, _Buf)

    src, dst = _Buf(input, False), _Buf(output, True)
    if src.nbytes % BLOCK_BYTES[fmt] != 0:
        raise InvalidLength(src.nbytes)
    if dst.nbytes < src.nbytes:
        raise OutputBufferTooSmall(src.nbytes, dst.nbytes)
    if (src.device is None) != (dst.device is None):
        raise TypeError("input and output must both be host buffers or both be device tensors")
    l = _l()
    mode, sa, sc = C.c_uint8(), C.c_bool(), C.c_bool()
    outs = {"bc1": (C.byref(mode), C.byref(sc)), "bc2": (C.byref(mode), C.byref(sc)), "bc3": (C.byref(mode), C.byref(sa), C.byref(sc)),
            "bc4": (C.byref(sa),), "bc5": (C.byref(sa),)}[fmt]
    use_all = bool(use_all_decorrelation_modes)
    if src.device is None:
        f = getattr(l, f"dxtlt_transform_{fmt}_auto")
        if fmt in ("bc4", "bc5"):
            rc = f(src.ptr, dst.ptr, src.nbytes, builtin_size_estimator(), *outs)
        else:
            rc = f(src.ptr, dst.ptr, src.nbytes, builtin_size_estimator(), use_all, *outs, None)
    else:
        import torch

        with torch.cuda.device(src.device):
            rc = getattr(l, f"dxtlt_transform_{fmt}_auto_device")(src.ptr, dst.ptr, src.nbytes, use_all,
                                                                  torch.cuda.current_stream().cuda_stream, *outs)
    _check(rc)
    if fmt == "bc1":
        return Bc1TransformSettings(YCoCgVariant(mode.value), sc.value)
    if fmt == "bc2":
        return Bc2TransformSettings(YCoCgVariant(mode.value), sc.value)
    if fmt == "bc3":
        return Bc3TransformSettings(YCoCgVariant(mode.value), sa.value, sc.value)
    return (Bc4TransformSettings if fmt == "bc4" else Bc5TransformSettings)(sa.value)


def _settings_of(fmt: str, mode: int, sa: int, sc: int):
    from . import (Bc1TransformSettings, Bc2TransformSettings, Bc3TransformSettings, Bc4TransformSettings, Bc5TransformSettings,
                   YCoCgVariant)

    if fmt == "bc1":
        return Bc1TransformSettings(YCoCgVariant(mode), bool(sc))
    if fmt == "bc2":
        return Bc2TransformSettings(YCoCgVariant(mode), bool(sc))
    if fmt == "bc3":
        return Bc3TransformSettings(YCoCgVariant(mode), bool(sa), bool(sc))
    return (Bc4TransformSettings if fmt == "bc4" else Bc5TransformSettings)(bool(sa))


def transform_batch_auto(items):
    """dxtlt_transform_batch_auto_device: items are (fmt, input tensor, output tensor, use_all_decorrelation_modes) with fmt in
    bc1..bc5 and CUDA uint8 tensors on one device.  Chooses the best settings for every item with the built-in estimator and
    transforms them all on torch's current stream: one stream wait and a launch count that does not grow with the number of
    items.  Returns the list of chosen settings objects, one per item; the transforms are enqueued, not waited for."""
    import torch

    if not items:
        return []
    arr, device, _keep = _batch_auto_items("transform_batch_auto", items)
    with torch.cuda.device(device):
        _check(_l().dxtlt_transform_batch_auto_device(arr, len(arr), torch.cuda.current_stream().cuda_stream))
    return [_settings_of(fmt, a.decorrelation_mode, a.split_alpha_endpoints, a.split_colour_endpoints)
            for (fmt, _s, _d, _u), a in zip(items, arr)]


def _batch_auto_items(who: str, items):
    """(the DxtltBatchAutoItem array, the device, the buffers kept alive) of (fmt, input, output, use_all) items"""
    from . import _FMT_ID, BLOCK_BYTES, InvalidLength, OutputBufferTooSmall, _Buf

    arr = (BatchAutoItem * max(1, len(items)))()
    device, keep = None, []
    for k, (fmt, src, dst, use_all) in enumerate(items):
        s, d = _Buf(src, False), _Buf(dst, True)
        if s.device is None or d.device is None:
            raise TypeError(f"{who} takes device tensors")
        device = s.device if device is None else device
        if s.device != device or d.device != device:
            raise ValueError("all tensors of a batch must live on one device")
        if s.nbytes % BLOCK_BYTES[fmt] != 0:
            raise InvalidLength(s.nbytes)
        if d.nbytes < s.nbytes:
            raise OutputBufferTooSmall(s.nbytes, d.nbytes)
        arr[k].d_input, arr[k].d_output, arr[k].len = s.ptr, d.ptr, s.nbytes
        arr[k].format, arr[k].use_all_decorrelation_modes = _FMT_ID[fmt], int(bool(use_all))
        keep.append((s, d))
    return arr, device, keep


def auto_sections_bytes(fmt: str, nbytes: int, use_all_decorrelation_modes: bool = False) -> int:
    """Bytes of the candidate sections of an input of `nbytes`: the single call's arena and a batch item's slice."""
    from . import BLOCK_BYTES

    per_block = {"bc1": 16, "bc2": 16, "bc3": 20, "bc4": 4, "bc5": 8}[fmt]
    if use_all_decorrelation_modes and fmt in ("bc1", "bc2", "bc3"):
        per_block += 16
    return nbytes // BLOCK_BYTES[fmt] * per_block


def debug_auto_candidates_into(fmt: str, input, arena, use_all_decorrelation_modes: bool = False) -> None:
    """Test hook (dxtlt_debug_auto_candidates_into_device): the fused candidate kernel of transform_auto, fmt in bc1..bc3, from the
    CUDA uint8 tensor `input` into the caller's `arena` of auto_sections_bytes(...) or more, both on a 16-byte boundary.  Enqueued
    on torch's current stream, not waited for."""
    import torch

    from . import _FMT_ID, OutputBufferTooSmall, _Buf

    src, dst = _Buf(input, False), _Buf(arena, True)
    if src.device is None or dst.device is None:
        raise TypeError("debug_auto_candidates_into takes device tensors")
    need = auto_sections_bytes(fmt, src.nbytes, use_all_decorrelation_modes)
    if dst.nbytes < need:
        raise OutputBufferTooSmall(need, dst.nbytes)
    f = _l().dxtlt_debug_auto_candidates_into_device
    f.argtypes, f.restype = [C.c_int32, C.c_bool, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p], C.c_int32
    with torch.cuda.device(src.device):
        _check(f(_FMT_ID[fmt], bool(use_all_decorrelation_modes), src.ptr, src.nbytes, dst.ptr, dst.nbytes,
                 torch.cuda.current_stream().cuda_stream))


def debug_batch_candidates(items, chunk: int, arena) -> None:
    """Test hook (dxtlt_debug_batch_auto_candidates_device): the candidate launches of chunk `chunk` of transform_batch_auto over
    `items` -- (fmt, input tensor, output tensor, use_all), as there; no output is written -- into the caller's CUDA uint8 tensor
    `arena`: item k's sections at the arena_offset dxtlt_debug_plan_batch_auto reports for it.  Waits for torch's current stream."""
    import torch

    from . import _Buf

    arr, _device, _keep = _batch_auto_items("debug_batch_candidates", items)
    a = _Buf(arena, True)
    if a.device is None:
        raise TypeError("debug_batch_candidates takes a device tensor as its arena")
    f = _l().dxtlt_debug_batch_auto_candidates_device
    f.argtypes = [C.POINTER(BatchAutoItem), C.c_size_t, C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p]
    f.restype = C.c_int32
    with torch.cuda.device(a.device):
        _check(f(arr, len(items), int(chunk), a.ptr, a.nbytes, torch.cuda.current_stream().cuda_stream))


def last_batch_auto() -> tuple[int, int, int, int]:
    """(stream waits, chunks, candidate launches, estimator launches) of the last transform_batch_auto of this thread."""
    buf = (C.c_uint64 * 4)()
    _l().dxtlt_debug_batch_auto_last(buf)
    return tuple(int(v) for v in buf)


def last_auto_estimation() -> tuple[int, int]:
    """(section bytes downloaded, estimator callbacks) of the last auto transform called from this thread."""
    a, b = C.c_uint64(), C.c_uint64()
    _l().dxtlt_debug_auto_last_estimation(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def last_auto_totals() -> list[int]:
    """The totals the last built-in-estimator auto transform called from this thread compared, in candidate order."""
    buf = (C.c_uint64 * 192)()     # 192: normalize.transform_bc3_auto_with_normalization with every decorrelation mode
    n = _l().dxtlt_debug_auto_last_totals(buf, 192)
    return [int(v) for v in buf[:n]]
