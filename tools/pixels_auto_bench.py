#!/usr/bin/env python3
"""Measures the pixel auto transform (include/dxtlt_pixels.h, docs/PIXEL_FORMAT.md "The auto transform") and the entropy
estimator's kernel on one GPU and writes profiles/pixels_auto_bench.json.

Cells: RGBA at 256^2, 4096^2 and 16384^2 pixels and RGB at 4096^2, each in THREE fresh processes (a process draws its clocks and
its placement once: the spread between processes is part of the result).  Per cell and process, on bounded random walks made on
the device:
  * dxtlt_transform_pixels_auto_device end to end (wall clock around the call and the wait for the winner's transform), on the
    arena route and on the route of one transform per candidate (dxtlt_debug_auto_use_arena(0)), interleaved round by round;
  * the arena route's phases by HIP events (dxtlt_debug_pixels_auto_time_phases): candidate kernel, estimator, readback + winner.
And once per process of the last cell: the entropy kernel alone on a 4 GiB section of the same kind of data and on a constant one,
HIP events, as a fraction of the 8 TB/s peak on `len` bytes read.  Medians of the rounds; nothing here is a gate.

    python tools/pixels_auto_bench.py [--out profiles/pixels_auto_bench.json] [--small]"""
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
CELLS = [("RGBA 256^2", 4, 256), ("RGBA 4096^2", 4, 4096), ("RGBA 16384^2", 4, 16384), ("RGB 4096^2", 3, 4096)]
ROUNDS = 7


def walks(pixels, B, seed):
    """(pixels * B,) uint8 on the device: B independent random walks, steps in -2..2, modulo 256, interleaved"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((pixels, B), dtype=torch.uint8, device="cuda")
    for c in range(B):
        steps = torch.randint(-2, 3, (pixels,), generator=g, device="cuda", dtype=torch.int32)
        out[:, c] = (torch.cumsum(steps, 0, dtype=torch.int32) + 128).to(torch.uint8)
        del steps
    return out.reshape(-1)


def child(B, side, with_kernel, small):
    import torch

    from dxt_lossless_transform_amd import estimator, pixels

    l = estimator._l()
    l.dxtlt_debug_pixels_auto_time_phases.argtypes, l.dxtlt_debug_pixels_auto_time_phases.restype = [C.c_int32], None
    l.dxtlt_debug_pixels_auto_last_phase_ms.argtypes, l.dxtlt_debug_pixels_auto_last_phase_ms.restype = [C.POINTER(C.c_double)], None
    x = walks(side * side, B, 0xBE7C + side)
    y = torch.empty_like(x)

    def once(arena):
        l.dxtlt_debug_auto_use_arena(arena)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        choice = pixels.transform_auto(x, y, B)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, choice

    for arena in (1, 0):
        once(arena)                                             # warm-up: module load, arena and counter allocation
    arena_ms, fallback_ms, choices = [], [], set()
    for _ in range(ROUNDS):
        for arena, sink in ((1, arena_ms), (0, fallback_ms)):
            ms, choice = once(arena)
            sink.append(ms)
            choices.add(choice)
    l.dxtlt_debug_auto_use_arena(1)
    l.dxtlt_debug_pixels_auto_time_phases(1)
    phases = []
    for _ in range(ROUNDS):
        pixels.transform_auto(x, y, B)
        buf = (C.c_double * 3)()
        l.dxtlt_debug_pixels_auto_last_phase_ms(buf)
        phases.append(list(buf))
    l.dxtlt_debug_pixels_auto_time_phases(0)
    row = {"len_bytes": x.numel(), "choices": sorted(choices), "arena_ms": statistics.median(arena_ms), "arena_ms_min": min(arena_ms),
           "fallback_ms": statistics.median(fallback_ms), "fallback_ms_min": min(fallback_ms),
           "phase_ms": {k: statistics.median(p[i] for p in phases) for i, k in enumerate(("candidates", "estimator", "readback_winner"))}}
    row["fallback_over_arena"] = row["fallback_ms"] / row["arena_ms"]
    if with_kernel:
        del x, y
        n = (4 << 30) >> (6 if small else 0)
        out = torch.zeros(1, dtype=torch.int64, device="cuda")
        kernel = {}
        for kind in ("walks", "constant"):
            d = walks(n // 4, 4, 7) if kind == "walks" else torch.full((n,), 255, dtype=torch.uint8, device="cuda")
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            times = []
            for _ in range(ROUNDS + 1):
                a.record()
                estimator.estimate_entropy_sizes([d], out)
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b))
            ms = statistics.median(times[1:])
            kernel[kind] = {"len_bytes": n, "ms": ms, "fraction_of_8TBps": n / (ms * 1e-3) / PEAK, "estimate": int(out.item())}
            del d
        row["entropy_kernel_4GiB"] = kernel
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixels_auto_bench.json"))
    ap.add_argument("--small", action="store_true", help="sides capped at 2048 and a 64 MiB kernel section (a quick look, not the record)")
    ap.add_argument("--child", nargs=3, metavar=("B", "SIDE", "KERNEL"))
    args = ap.parse_args()
    if args.child:
        return child(int(args.child[0]), int(args.child[1]), args.child[2] == "1", args.small)
    cells = []
    for k, (name, B, side) in enumerate(CELLS):
        side = min(side, 2048) if args.small else side
        runs = []
        for _ in range(3):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), str(side), "1" if k == len(CELLS) - 1 else "0"]
            r = subprocess.run(cmd + (["--small"] if args.small else []), capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"{name}: child failed ({r.returncode})\n{r.stderr[-2000:]}")
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(name, {k2: runs[-1][k2] for k2 in ("arena_ms", "fallback_ms", "fallback_over_arena", "phase_ms")}, flush=True)
        cells.append({"cell": name, "pixel_bytes": B, "side": side, "processes": runs})
    import torch

    doc = {"tool": "pixels_auto_bench", "device": torch.cuda.get_device_name(0), "small": args.small, "rounds": ROUNDS, "cells": cells}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
