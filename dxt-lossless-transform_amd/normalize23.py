"""BC2 / BC3 block normalisation -- host-side mirror of the reference's experimental modules
(``dxt_lossless_transform_bc{2,3}::experimental::normalize_blocks``) over include/dxtlt_bc23_normalize.h.  numpy /
bytes-like host buffers or CUDA ``torch.uint8`` tensors (enqueued on torch's current stream).  No CPU fallback."""
from __future__ import annotations

import ctypes as C
import enum
from typing import Sequence

from .normalize import ColorNormalizationMode  # same three values in all formats
from .normalize import _bufs, _device_of, _run, _sized


class AlphaNormalizationMode(enum.IntEnum):
    """bc3 normalize.rs:117-139"""

    NONE = 0
    UNIFORM_ALPHA_ZERO_INDICES = 1
    OPAQUE_FILL_ALL = 2
    OPAQUE_ZERO_ALPHA_MAX_INDICES = 3


def normalize_blocks(fmt: str, input, output, color_mode: ColorNormalizationMode,
                     alpha_mode: AlphaNormalizationMode = AlphaNormalizationMode.NONE) -> None:
    """bc2 normalize.rs:35 / bc3 normalize.rs:36; ``output`` may be ``input`` (in place)."""
    assert fmt in ("bc2", "bc3")
    src, dst = _bufs((input, output), (False, True))
    device = _device_of((src, dst))
    _sized(src, dst, 16)
    modes = (int(color_mode),) if fmt == "bc2" else (int(alpha_mode), int(color_mode))
    _run(f"dxtlt_{fmt}_normalize_blocks", device, (src.ptr, dst.ptr, src.nbytes, *modes))


def normalize_blocks_all_modes(fmt: str, input, outputs: Sequence) -> None:
    """bc2 normalize.rs:193 (3 outputs, by colour mode) / bc3 normalize.rs:419 (12 outputs, [alpha_mode * 3 + colour_mode])."""
    from . import InvalidLength, OutputBufferTooSmall

    assert fmt in ("bc2", "bc3")
    count = 3 if fmt == "bc2" else 12
    if len(outputs) != count:
        raise ValueError(f"{count} output buffers are required")
    src, *outs = _bufs((input, *outputs), (False,) + (True,) * count)
    device = _device_of((src, *outs))
    if src.nbytes % 16 != 0:
        raise InvalidLength(src.nbytes)
    for o in outs:
        if o.nbytes < src.nbytes:
            raise OutputBufferTooSmall(src.nbytes, o.nbytes)
    ptrs = (C.c_void_p * count)(*[o.ptr for o in outs])
    _run(f"dxtlt_{fmt}_normalize_blocks_all_modes", device, (src.ptr, ptrs, src.nbytes))


def normalize_bc2_split_blocks_in_place(alpha, colors, indices, color_mode: ColorNormalizationMode) -> None:
    """bc2 normalize.rs:382.  ``alpha`` (8 bytes per block) is accepted for signature parity and may be None."""
    from . import InvalidLength

    c, x = _bufs((colors, indices), (True, True))
    device = _device_of((c, x))
    if c.nbytes % 4 != 0 or c.nbytes != x.nbytes:
        raise InvalidLength(c.nbytes)
    args = (c.ptr, x.ptr, c.nbytes // 4, int(color_mode))
    _run("dxtlt_bc2_normalize_split_blocks_in_place", device, (None, *args), args)


def normalize_bc3_split_blocks_in_place(alpha_endpoints, alpha_indices, color_endpoints, color_indices,
                                        alpha_mode: AlphaNormalizationMode, color_mode: ColorNormalizationMode) -> None:
    """bc3 normalize.rs:539: sections of 2, 6, 4 and 4 bytes per block, all modified in place."""
    from . import InvalidLength

    ae, ai, ce, ci = _bufs((alpha_endpoints, alpha_indices, color_endpoints, color_indices), (True,) * 4)
    device = _device_of((ae, ai, ce, ci))
    n = ae.nbytes // 2
    if ae.nbytes != 2 * n or ai.nbytes != 6 * n or ce.nbytes != 4 * n or ci.nbytes != 4 * n:
        raise InvalidLength(ae.nbytes)
    _run("dxtlt_bc3_normalize_split_blocks_in_place", device, (ae.ptr, ai.ptr, ce.ptr, ci.ptr, n, int(alpha_mode), int(color_mode)))
