#!/usr/bin/env python3
"""Measures the batched pixel calls (include/dxtlt_pixels.h; docs/PIXEL_FORMAT.md "Many buffers in one call") on one GPU against
loops of the single-buffer calls and writes profiles/pixels_batch_bench.json.

Cells: 8000 mip chains of 256^2, 1024 of 1024^2 and 64 of 4096^2 RGBA pixels, and 8000 chains of 256^2 RGB pixels, each in THREE
fresh processes (a process draws its clocks and its placement once: the spread between processes is part of the result).  The
data is bounded random walks made on the device; every chain starts on a 256-byte boundary of one allocation.  Per cell and
process, interleaved round by round, host clock around the call(s) and the device synchronise behind them:
  * dxtlt_transform_pixels_batch_device, forward and inverse at the default setting (decorrelate, PLANAR_DELTA), next to a loop
    of dxtlt_transform_pixels_device / dxtlt_untransform_pixels_device over the same buffers;
  * dxtlt_transform_pixels_batch_auto_device next to a loop of dxtlt_transform_pixels_auto_device;
  * the phases of the batched auto call by HIP events (dxtlt_debug_pixels_batch_auto_time_phases);
  * the manual batch's end-to-end rate on 2 x len bytes as a fraction of the 8 TB/s peak, and beside it, in the same process, the
    single-buffer call on ONE buffer (4 GiB, or all the cell's bytes when that is less).  Whole-call rates, not kernel times.
Medians of the rounds; nothing here is a gate.

    python tools/pixels_batch_bench.py [--out profiles/pixels_batch_bench.json] [--small]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
CELLS = [("8000 x 256^2 chains RGBA", 4, 256, 8000), ("1024 x 1024^2 chains RGBA", 4, 1024, 1024), ("64 x 4096^2 chains RGBA", 4, 4096, 64),
         ("8000 x 256^2 chains RGB", 3, 256, 8000)]
ROUNDS = 5


def chain_pixels(side):
    n = 0
    while side >= 1:
        n += side * side
        side //= 2
    return n


def walks(pixels, B, seed):
    """(pixels * B,) uint8 on the device: B independent random walks, steps in -2..2, reflected into +-120 around 128, interleaved"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((pixels, B), dtype=torch.uint8, device="cuda")
    for c in range(B):
        steps = torch.randint(-2, 3, (pixels,), generator=g, device="cuda", dtype=torch.int32)
        w = torch.cumsum(steps, 0, dtype=torch.int64)
        out[:, c] = (((w + 120) % 480 - 240).abs() - 120 + 128).to(torch.uint8)
        del steps, w
    return out.reshape(-1)


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def child(B, side, count):
    import torch

    from dxt_lossless_transform_amd import _lib, pixels

    l = pixels._l()
    l.dxtlt_debug_pixels_batch_auto_time_phases.argtypes, l.dxtlt_debug_pixels_batch_auto_time_phases.restype = [C.c_int32], None
    l.dxtlt_debug_pixels_batch_auto_last_phase_ms.argtypes = [C.POINTER(C.c_double)]
    l.dxtlt_debug_pixels_batch_auto_last_phase_ms.restype = None
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
    l.dxtlt_transform_pixels_batch_device.argtypes, l.dxtlt_transform_pixels_batch_device.restype = [C.POINTER(pixels.PixelBatchItem), sz, vp], i32
    l.dxtlt_transform_pixels_batch_auto_device.argtypes = [C.POINTER(pixels.PixelBatchAutoItem), sz, vp]
    l.dxtlt_transform_pixels_batch_auto_device.restype = i32
    l.dxtlt_transform_pixels_auto_device.argtypes = [vp, vp, sz, i32, vp, C.POINTER(C.c_bool), C.POINTER(C.c_uint8)]
    l.dxtlt_transform_pixels_auto_device.restype = i32
    P = chain_pixels(side)
    n = P * B
    stride = (n + 255) & ~255                                   # every chain on a 256-byte boundary, as separate allocations would be
    x = torch.zeros(stride * count, dtype=torch.uint8, device="cuda")
    x.view(count, stride)[:, :n] = walks(P * count, B, 0xBA7C + side).view(count, n)
    y, z = torch.zeros_like(x), torch.zeros_like(x)
    stream = torch.cuda.current_stream().cuda_stream
    # the C calls themselves, on arrays and addresses made once: no Python wrapper inside a timed window
    xp, yp, zp = ([t.data_ptr() + k * stride for k in range(count)] for t in (x, y, z))
    forward, inverse = (pixels.PixelBatchItem * count)(), (pixels.PixelBatchItem * count)()
    autos = (pixels.PixelBatchAutoItem * count)()
    for k in range(count):
        forward[k].d_input, forward[k].d_output, inverse[k].d_input, inverse[k].d_output = xp[k], yp[k], yp[k], zp[k]
        autos[k].d_input, autos[k].d_output, autos[k].len, autos[k].pixel_bytes = xp[k], zp[k], n, B
        for it, inv in ((forward[k], 0), (inverse[k], 1)):
            it.len, it.pixel_bytes, it.inverse, it.decorrelate, it.layout = n, B, inv, 1, pixels.PLANAR_DELTA

    def ok(rc):
        assert rc == 0, _lib.last_error()

    def loop_forward():
        for k in range(count):
            ok(l.dxtlt_transform_pixels_device(xp[k], yp[k], n, B, True, pixels.PLANAR_DELTA, stream))

    def loop_inverse():
        for k in range(count):
            ok(l.dxtlt_untransform_pixels_device(yp[k], zp[k], n, B, True, pixels.PLANAR_DELTA, stream))

    dec, lay = C.c_bool(), C.c_uint8()

    def loop_auto():
        for k in range(count):
            ok(l.dxtlt_transform_pixels_auto_device(xp[k], zp[k], n, B, stream, C.byref(dec), C.byref(lay)))

    def batch_auto():
        ok(l.dxtlt_transform_pixels_batch_auto_device(autos, count, stream))

    work = {"batch_forward": lambda: ok(l.dxtlt_transform_pixels_batch_device(forward, count, stream)), "loop_forward": loop_forward,
            "batch_inverse": lambda: ok(l.dxtlt_transform_pixels_batch_device(inverse, count, stream)), "loop_inverse": loop_inverse,
            "batch_auto": batch_auto, "loop_auto": loop_auto}
    for fn in work.values():
        fn()                                                     # warm-up: module load, table slots, arena and counters
    torch.cuda.synchronize()
    ok(l.dxtlt_transform_pixels_batch_device(inverse, count, stream))
    torch.cuda.synchronize()
    assert torch.equal(x, z), "the inverse batch does not restore the input"
    ms = {k: [] for k in work}
    for _ in range(ROUNDS):
        for k, fn in work.items():
            ms[k].append(timed(fn))
    l.dxtlt_debug_pixels_batch_auto_time_phases(1)
    phases = []
    for _ in range(ROUNDS):
        batch_auto()
        buf = (C.c_double * 3)()
        l.dxtlt_debug_pixels_batch_auto_last_phase_ms(buf)
        phases.append(list(buf))
    l.dxtlt_debug_pixels_batch_auto_time_phases(0)
    # one buffer through the single-buffer call, in the same process: the cell's bytes, at most 4 GiB
    one = min(x.numel(), 4 << 30) // (B * 4096) * (B * 4096)
    single = [timed(lambda: pixels.transform_pixels(x[:one], y[:one], B)) for _ in range(ROUNDS + 1)][1:]
    total = n * count
    row = {"len_bytes": total, "items": count, "item_bytes": n, "auto_choices": sorted({(int(a.decorrelate), int(a.layout)) for a in autos})}
    for k, v in ms.items():
        row[k + "_ms"] = statistics.median(v)
        row[k + "_ms_min"] = min(v)
    for kind in ("forward", "inverse", "auto"):
        row[f"loop_over_batch_{kind}"] = row[f"loop_{kind}_ms"] / row[f"batch_{kind}_ms"]
    row["auto_phase_ms"] = {k: statistics.median(p[i] for p in phases) for i, k in enumerate(("candidates", "estimator", "winners"))}
    row["batch_forward_fraction_of_8TBps"] = 2 * total / (row["batch_forward_ms"] * 1e-3) / PEAK
    row["batch_inverse_fraction_of_8TBps"] = 2 * total / (row["batch_inverse_ms"] * 1e-3) / PEAK
    row["single_buffer"] = {"len_bytes": one, "ms": statistics.median(single), "fraction_of_8TBps": 2 * one / (statistics.median(single) * 1e-3) / PEAK}
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixels_batch_bench.json"))
    ap.add_argument("--small", action="store_true", help="a sixteenth of every cell's items (a quick look, not the record)")
    ap.add_argument("--child", nargs=3, metavar=("B", "SIDE", "COUNT"))
    args = ap.parse_args()
    if args.child:
        return child(*(int(v) for v in args.child))
    cells = []
    for name, B, side, count in CELLS:
        count = max(1, count // 16) if args.small else count
        runs = []
        for _ in range(3):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), str(side), str(count)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"{name}: child failed ({r.returncode})\n{r.stderr[-2000:]}")
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(name, {k: round(runs[-1][k], 3) for k in runs[-1] if k.startswith("loop_over_batch") or k.endswith("fraction_of_8TBps")},
                  runs[-1]["single_buffer"], flush=True)
        cells.append({"cell": name, "pixel_bytes": B, "side": side, "items": count, "processes": runs})
    import torch

    doc = {"tool": "pixels_batch_bench", "device": torch.cuda.get_device_name(0), "small": args.small, "rounds": ROUNDS, "cells": cells}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
