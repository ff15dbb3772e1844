"""BC1 block normalisation -- host-side mirror of the reference's experimental module
(``dxt_lossless_transform_bc1::experimental::normalize_blocks``, normalize.rs / transform.rs / mod.rs) over the C ABI of
include/dxtlt_bc1_normalize.h.  Same buffer conventions as the BC1-3 functions: numpy/bytes-like host buffers or CUDA
``torch.uint8`` tensors (device path, enqueued on torch's current stream).  No CPU fallback.  normalize23.py (BC2 / BC3) shares
this module's prototype table and its buffer, size and call helpers."""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
from typing import Iterator, Sequence

from . import _lib


class ColorNormalizationMode(enum.IntEnum):
    """normalize.rs:487-500"""

    NONE = 0
    COLOR0_ONLY = 1
    REPLICATE_COLOR = 2


@dataclasses.dataclass(frozen=True)
class Bc1TransformDetailsWithNormalization:
    """experimental/normalize_blocks/mod.rs:98-113; defaults :126-135"""

    color_normalization_mode: ColorNormalizationMode = ColorNormalizationMode.NONE
    decorrelation_mode: int = 1  # core YCoCgVariant numbering, Variant1
    split_colour_endpoints: bool = True

    @staticmethod
    def all_combinations() -> Iterator["Bc1TransformDetailsWithNormalization"]:
        # mod.rs:170-184: mode-major, then decorrelation (None, Variant1..3), then split true / false
        for m in ColorNormalizationMode:
            for v in (0, 1, 2, 3):
                for s in (True, False):
                    yield Bc1TransformDetailsWithNormalization(m, v, s)

    def untransform_settings(self):
        """`impl From<Bc1TransformDetailsWithNormalization> for Bc1UntransformSettings` (mod.rs:115-122)."""
        from . import Bc1TransformSettings, YCoCgVariant

        return Bc1TransformSettings(YCoCgVariant(self.decorrelation_mode), self.split_colour_endpoints)


# One table of prototypes for both headers.  A `_device` twin takes the same arguments and a trailing stream unless it is listed.
_VP, _SZ, _U8, _B = C.c_void_p, C.c_size_t, C.c_uint8, C.c_bool
_PP = C.POINTER(_VP)
_HOST = {
    # include/dxtlt_bc1_normalize.h
    "dxtlt_bc1_normalize_blocks": [_VP, _VP, _SZ, _U8],
    "dxtlt_bc1_normalize_split_blocks_in_place": [_VP, _VP, _SZ, _U8],
    "dxtlt_bc1_normalize_blocks_all_modes": [_VP, _PP, _SZ, C.POINTER(_B)],
    "dxtlt_transform_bc1_with_normalize_blocks": [_VP, _VP, _VP, _SZ, _U8, _U8, _B],
    # include/dxtlt_bc23_normalize.h
    "dxtlt_bc2_normalize_blocks": [_VP, _VP, _SZ, _U8],
    "dxtlt_bc3_normalize_blocks": [_VP, _VP, _SZ, _U8, _U8],
    "dxtlt_bc2_normalize_split_blocks_in_place": [_VP, _VP, _VP, _SZ, _U8],
    "dxtlt_bc3_normalize_split_blocks_in_place": [_VP, _VP, _VP, _VP, _SZ, _U8, _U8],
    "dxtlt_bc2_normalize_blocks_all_modes": [_VP, _PP, _SZ],
    "dxtlt_bc3_normalize_blocks_all_modes": [_VP, _PP, _SZ],
    "dxtlt_transform_bc2_with_normalize_blocks": [_VP, _VP, _SZ, _U8, _U8, _B],
    "dxtlt_transform_bc3_with_normalize_blocks": [_VP, _VP, _SZ, _U8, _U8, _U8, _B, _B],
}
_DEVICE = {   # the twins that differ: no work_ptr, a device flag word, no alpha array
    "dxtlt_transform_bc1_with_normalize_blocks_device": [_VP, _VP, _SZ, _U8, _U8, _B, _VP],
    "dxtlt_bc1_normalize_blocks_all_modes_device": [_VP, _PP, _SZ, _VP, _VP],
    "dxtlt_bc2_normalize_split_blocks_in_place_device": [_VP, _VP, _SZ, _U8, _VP],
}
_declared = False


def _l():
    global _declared
    l = _lib.load()
    if not _declared:
        for name, args in _HOST.items():
            getattr(l, name).argtypes, getattr(l, name).restype = args, C.c_int32
            twin = getattr(l, name + "_device")
            twin.argtypes, twin.restype = _DEVICE.get(name + "_device", args + [_VP]), C.c_int32
        _declared = True
    return l


def _bufs(items, writable):
    from . import _Buf

    return [_Buf(x, w) for x, w in zip(items, writable)]


def _device_of(bufs, mismatch="all buffers must be host buffers or all be tensors on one device"):
    """None for host buffers, the device index for tensors; every buffer in the same place"""
    if len({b.device for b in bufs}) != 1:
        raise TypeError(mismatch)
    return bufs[0].device


def _sized(src, dst, block: int) -> None:
    from . import InvalidLength, OutputBufferTooSmall

    if src.nbytes % block != 0:
        raise InvalidLength(src.nbytes)
    if dst.nbytes < src.nbytes:
        raise OutputBufferTooSmall(src.nbytes, dst.nbytes)


def _run(name: str, device, host_args, device_args=None) -> None:
    """The host entry point `name`, or -- for tensors -- its _device twin on their device and torch's current stream."""
    from . import _check

    if device is None:
        _check(getattr(_l(), name)(*host_args))
    else:
        import torch

        with torch.cuda.device(device):
            args = host_args if device_args is None else device_args
            _check(getattr(_l(), name + "_device")(*args, torch.cuda.current_stream(device).cuda_stream))


def normalize_blocks(input, output, color_mode: ColorNormalizationMode) -> None:
    """normalize.rs:38.  ``output`` may be the same buffer as ``input`` (in place)."""
    src, dst = _bufs((input, output), (False, True))
    _sized(src, dst, 8)
    device = _device_of((src, dst), "input and output must both be host buffers or both be device tensors")
    _run("dxtlt_bc1_normalize_blocks", device, (src.ptr, dst.ptr, src.nbytes, int(color_mode)))


def normalize_split_blocks_in_place(colors, indices, color_mode: ColorNormalizationMode) -> None:
    """normalize.rs:286: colours (4 bytes per block) and indices (4 bytes per block), both modified in place."""
    from . import InvalidLength

    c, x = _bufs((colors, indices), (True, True))
    if c.nbytes % 4 != 0 or c.nbytes != x.nbytes:
        raise InvalidLength(c.nbytes)
    device = _device_of((c, x), "colors and indices must both be host buffers or both be device tensors")
    _run("dxtlt_bc1_normalize_split_blocks_in_place", device, (c.ptr, x.ptr, c.nbytes // 4, int(color_mode)))


def normalize_blocks_all_modes(input, outputs: Sequence) -> bool:
    """normalize.rs:417: one output per ColorNormalizationMode, in enum order.  Returns whether any block was
    normalised.  Device tensors: synchronises the current stream to read the flag."""
    from . import InvalidLength, OutputBufferTooSmall

    if len(outputs) != len(ColorNormalizationMode):
        raise ValueError("one output buffer per ColorNormalizationMode is required")
    src, *outs = _bufs((input, *outputs), (False, True, True, True))
    if src.nbytes % 8 != 0:
        raise InvalidLength(src.nbytes)
    for o in outs:
        if o.nbytes < src.nbytes:
            raise OutputBufferTooSmall(src.nbytes, o.nbytes)
        _device_of((src, o), "input and outputs must all be host buffers or all be device tensors")
    ptrs = (C.c_void_p * 3)(*[o.ptr for o in outs])
    name = "dxtlt_bc1_normalize_blocks_all_modes"
    if src.device is None:
        flag = C.c_bool(False)
        _run(name, None, (src.ptr, ptrs, src.nbytes, C.byref(flag)))
        return bool(flag.value)
    import torch

    with torch.cuda.device(src.device):
        any_word = torch.zeros(1, dtype=torch.int32, device=input.device)
        _run(name, src.device, (src.ptr, ptrs, src.nbytes, any_word.data_ptr()))
        return bool(any_word.item() != 0)


def transform_bc1_with_normalize_blocks(input, output,
                                        details: Bc1TransformDetailsWithNormalization = Bc1TransformDetailsWithNormalization(),
                                        ) -> None:
    """transform.rs:65 (the reference's ``work_ptr`` scratch buffer has no counterpart: normalisation is fused into
    the transform kernel).  Undo with ``untransform_bc1_with_settings(..., details.untransform_settings())``."""
    src, dst = _bufs((input, output), (False, True))
    _sized(src, dst, 8)
    device = _device_of((src, dst), "input and output must both be host buffers or both be device tensors")
    args = (int(details.color_normalization_mode), int(details.decorrelation_mode), bool(details.split_colour_endpoints))
    _run("dxtlt_transform_bc1_with_normalize_blocks", device, (src.ptr, dst.ptr, None, src.nbytes, *args),
         (src.ptr, dst.ptr, src.nbytes, *args))


def _fused_bc23(fmt: str, input, output, mode_args: tuple, settings_args: tuple) -> None:
    src, dst = _bufs((input, output), (False, True))
    _sized(src, dst, 16)
    device = _device_of((src, dst), "input and output must both be host buffers or both be device tensors")
    _run(f"dxtlt_transform_{fmt}_with_normalize_blocks", device, (src.ptr, dst.ptr, src.nbytes, *mode_args, *settings_args))


def transform_bc2_with_normalize_blocks(input, output, color_mode: ColorNormalizationMode, decorrelation_mode: int = 1,
                                        split_colour_endpoints: bool = True) -> None:
    """``transform_bc2_with_settings(normalize_blocks(input, color_mode), settings)`` in one pass, normalisation fused into the
    transform kernel (include/dxtlt_bc23_normalize.h; upstream has no such function).  ``decorrelation_mode`` in the core
    YCoCgVariant numbering.  Undo with ``untransform_bc2_with_settings``: it yields the normalised blocks."""
    _fused_bc23("bc2", input, output, (int(color_mode),), (int(decorrelation_mode), bool(split_colour_endpoints)))


def transform_bc3_with_normalize_blocks(input, output, alpha_mode, color_mode: ColorNormalizationMode, decorrelation_mode: int = 1,
                                        split_alpha_endpoints: bool = True, split_colour_endpoints: bool = True) -> None:
    """``transform_bc3_with_settings(normalize_blocks(input, alpha_mode, color_mode), settings)`` in one pass; ``alpha_mode`` is a
    ``normalize23.AlphaNormalizationMode``.  Undo with ``untransform_bc3_with_settings``: it yields the normalised blocks."""
    _fused_bc23("bc3", input, output, (int(alpha_mode), int(color_mode)),
                (int(decorrelation_mode), bool(split_alpha_endpoints), bool(split_colour_endpoints)))


# ---- the auto transform with block normalisation (include/dxtlt_auto_normalize.h; docs/ESTIMATOR.md) ---------------------------------
_auto_declared = False


def _auto_l():
    global _auto_declared
    l = _l()
    if not _auto_declared:
        u8p, bp = C.POINTER(_U8), C.POINTER(_B)
        for fmt in ("bc1", "bc2"):
            f = getattr(l, f"dxtlt_transform_{fmt}_auto_with_normalization")
            f.argtypes, f.restype = [_VP, _VP, _SZ, _VP, _B, u8p, u8p, bp, C.POINTER(C.c_uint32)], C.c_int32
            f = getattr(l, f"dxtlt_transform_{fmt}_auto_with_normalization_device")
            f.argtypes, f.restype = [_VP, _VP, _SZ, _B, _VP, u8p, u8p, bp], C.c_int32
        l.dxtlt_transform_bc3_auto_with_normalization.argtypes = [_VP, _VP, _SZ, _VP, _B, u8p, u8p, u8p, bp, bp, C.POINTER(C.c_uint32)]
        l.dxtlt_transform_bc3_auto_with_normalization.restype = C.c_int32
        l.dxtlt_transform_bc3_auto_with_normalization_device.argtypes = [_VP, _VP, _SZ, _B, _VP, u8p, u8p, u8p, bp, bp]
        l.dxtlt_transform_bc3_auto_with_normalization_device.restype = C.c_int32
        _auto_declared = True
    return l


def _auto_with_normalization(fmt: str, input, output, estimator, use_all_decorrelation_modes: bool):
    from . import _check

    src, dst = _bufs((input, output), (False, True))
    _sized(src, dst, 8 if fmt == "bc1" else 16)
    device = _device_of((src, dst), "input and output must both be host buffers or both be device tensors")
    l = _auto_l()
    alpha, norm, mode, split_alpha, split = _U8(), _U8(), _U8(), _B(), _B()
    outs = (C.byref(norm), C.byref(mode), C.byref(split))
    if fmt == "bc3":
        outs = (C.byref(alpha), C.byref(norm), C.byref(mode), C.byref(split_alpha), C.byref(split))
    use_all = bool(use_all_decorrelation_modes)
    if device is None:
        if estimator is None:
            from . import estimator as _estimator

            estimator = _estimator.builtin_size_estimator()
        elif isinstance(estimator, C.Structure):
            estimator = C.cast(C.pointer(estimator), _VP)
        _check(getattr(l, f"dxtlt_transform_{fmt}_auto_with_normalization")(src.ptr, dst.ptr, src.nbytes, estimator, use_all, *outs, None))
    else:
        if estimator is not None:
            raise TypeError("device tensors are estimated with the built-in estimator: pass no estimator")
        import torch

        with torch.cuda.device(device):
            _check(getattr(l, f"dxtlt_transform_{fmt}_auto_with_normalization_device")(
                src.ptr, dst.ptr, src.nbytes, use_all, torch.cuda.current_stream(device).cuda_stream, *outs))
    if fmt == "bc3":
        return int(alpha.value), ColorNormalizationMode(norm.value), int(mode.value), bool(split_alpha.value), bool(split.value)
    return ColorNormalizationMode(norm.value), int(mode.value), bool(split.value)


def transform_bc1_auto_with_normalization(input, output, estimator=None, use_all_decorrelation_modes: bool = False,
                                          ) -> Bc1TransformDetailsWithNormalization:
    """transform.rs:222: the colour normalisation mode and the transform settings whose colour section the estimator finds
    smallest; ``output`` holds ``transform_bc1_with_normalize_blocks(input, result)``.  Host buffers (``estimator``: a
    ``DltSizeEstimator`` structure or a pointer to one; None: the built-in estimator, everything on the device) or CUDA
    ``torch.uint8`` tensors (the built-in estimator, on torch's current stream, which the call waits for twice)."""
    return Bc1TransformDetailsWithNormalization(*_auto_with_normalization("bc1", input, output, estimator, use_all_decorrelation_modes))


def transform_bc2_auto_with_normalization(input, output, estimator=None, use_all_decorrelation_modes: bool = False):
    """BC2's twin (this build's extension, include/dxtlt_auto_normalize.h).  Returns (ColorNormalizationMode, decorrelation mode in
    the core YCoCgVariant numbering, split_colour_endpoints); ``output`` holds ``transform_bc2_with_normalize_blocks`` with them."""
    return _auto_with_normalization("bc2", input, output, estimator, use_all_decorrelation_modes)


def transform_bc3_auto_with_normalization(input, output, estimator=None, use_all_decorrelation_modes: bool = False):
    """BC3's twin (this build's extension, include/dxtlt_auto_normalize.h): 4 alpha modes x 3 colour modes x BC3's 8 / 16 settings,
    each the sum of its alpha and colour endpoint sections' estimates.  Returns (normalize23.AlphaNormalizationMode,
    ColorNormalizationMode, decorrelation mode in the core YCoCgVariant numbering, split_alpha_endpoints, split_colour_endpoints);
    ``output`` holds ``transform_bc3_with_normalize_blocks`` with them."""
    from .normalize23 import AlphaNormalizationMode

    alpha, norm, mode, split_alpha, split = _auto_with_normalization("bc3", input, output, estimator, use_all_decorrelation_modes)
    return AlphaNormalizationMode(alpha), norm, mode, split_alpha, split
