#!/usr/bin/env python3
"""Measures the uncompressed-pixel kernels (include/dxtlt_pixels.h, docs/PIXEL_FORMAT.md) on one GPU and writes
profiles/pixels_bench.json:

  * 4 GiB buffers of random bytes, both pixel sizes, all six settings, forward and inverse, at a pixel count P that is a
    multiple of 4096 (every access 16-byte aligned: the fast form) and at P + 1 (plane c starts at residue c mod 16 and the
    last tile is one pixel: the general form);
  * every cell timed with device events after a warm-up, reported as bytes moved (2 x len) per second and as a fraction of
    the 8 TB/s peak; every cell's round trip must be exact and three sampled tiles (first, middle, last whole one) of its
    forward output must equal tests/pixels_ref.py;
  * in the same run and through the same timing code, BC3 with default settings at the same byte size: the yardstick, a
    de-interleave with byte-granular streams that the library already carries.

    python tools/pixels_bench.py [--out profiles/pixels_bench.json] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dxt_lossless_transform_amd as pkg  # noqa: E402
import pixels_ref as R  # noqa: E402
from dxt_lossless_transform_amd import pixels  # noqa: E402

PEAK = 8.0e12
LAYOUT_NAMES = ("INTERLEAVED", "PLANAR", "PLANAR_DELTA")


def timed(fn, min_seconds=0.3, warm_seconds=0.1):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_seconds:
        fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 0, 0.0
    while total < min_seconds:
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b) / 1e3
        n += 1
    return total / n


def sampled_tiles_match(x, y, P, B, decorrelate, layout):
    for tile in (0, (P // 4096) // 2, P // 4096 - 1):
        first = tile * 4096
        want = R.forward(x[first * B:(first + 4096) * B].cpu().numpy(), B, decorrelate, layout)
        if layout == R.INTERLEAVED:
            got = y[first * B:(first + 4096) * B].cpu().numpy()
        else:
            got = np.concatenate([y[c * P + first:c * P + first + 4096].cpu().numpy() for c in range(B)])
        if not np.array_equal(got, want):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixels_bench.json"))
    ap.add_argument("--small", action="store_true", help="1/64 of the size (a quick look, not the record)")
    args = ap.parse_args()
    budget = (4 << 30) // (64 if args.small else 1)
    dev = torch.device("cuda:0")
    pkg.build()
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK, "buffer_bytes": budget, "cells": []}

    base = [torch.empty(budget + 64, dtype=torch.uint8, device=dev) for _ in range(3)]
    pkg.fill_splitmix64(base[0][:budget], 0x91E5)
    base[0][budget:] = 7

    # the yardstick: BC3, default settings, the same bytes
    x, y = base[0][:budget], base[1][:budget]
    dt = timed(lambda: pkg.transform_bc3_with_settings(x, y))
    dti = timed(lambda: pkg.untransform_bc3_with_settings(y, base[2][:budget]))
    res["bc3_default"] = {"bytes": budget, "forward_seconds": dt, "forward_fraction_of_peak": 2 * budget / dt / PEAK,
                          "inverse_seconds": dti, "inverse_fraction_of_peak": 2 * budget / dti / PEAK}
    print(res["bc3_default"], flush=True)

    for B in (4, 3):
        aligned = budget // B // 4096 * 4096
        for P in (aligned, aligned + 1):
            n = P * B
            x, y, z = (b[:n] for b in base)
            for decorrelate, layout in R.SETTINGS:
                fwd = timed(lambda: pixels.transform_pixels(x, y, B, decorrelate, layout))
                inv = timed(lambda: pixels.untransform_pixels(y, z, B, decorrelate, layout))
                torch.cuda.synchronize()
                cell = {"pixel_bytes": B, "pixels": P, "aligned": P == aligned, "decorrelate": decorrelate, "layout": LAYOUT_NAMES[layout],
                        "bytes": n, "forward_seconds": fwd, "forward_fraction_of_peak": 2 * n / fwd / PEAK, "inverse_seconds": inv,
                        "inverse_fraction_of_peak": 2 * n / inv / PEAK, "round_trip_exact": bool(torch.equal(z, x)),
                        "sampled_tiles_match_reference": sampled_tiles_match(x, y, P, B, decorrelate, layout)}
                res["cells"].append(cell)
                print(cell, flush=True)
                z.zero_()
    res["all_exact"] = all(c["round_trip_exact"] and c["sampled_tiles_match_reference"] for c in res["cells"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out, "all exact:", res["all_exact"])
    return 0 if res["all_exact"] else 1


if __name__ == "__main__":
    sys.exit(main())
