#!/usr/bin/env python3
"""Fused untransform + image decode (include/dxtlt_image.h) against the two calls it replaces.

Per format (BC1, BC2, BC3, default settings) and per block count (the image's own: aligned tiles; one extra block in the
transformed buffer, so that total_blocks is odd: shifted tiles), HIP-event times after a warm-up of
  (a) dxtlt_untransform_decode_image_device                                     -- must move len + 4 w h bytes
  (b) dxtlt_untransform_bcN_with_settings_device + dxtlt_decode_bcN_blocks_device into a scratch buffer
                                                                                -- must move 3 len + 64 blocks bytes
and the fraction of the 8 TB/s HBM peak each reaches on those bytes.  Before a cell is timed, three rows of (a)'s image are
compared with the CPU oracle.  Every cell is measured in `--processes` fresh processes (page placement moves a result by
0.02-0.03 of peak from one process to the next); the file keeps every sample, the median and the spread.

    python tools/image_decode_bench.py [--size 16384] [--steps 1000] [--processes 3] [--out profiles/image_decode_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8e12
FMT_ID = {"bc1": 1, "bc2": 2, "bc3": 3}
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16}
MODE, SA, SC = 1, True, True   # the settings types' defaults


def child(size, steps):
    """one process: every cell once; prints one JSON line"""
    import time

    import numpy as np
    import torch

    import dxt_lossless_transform_amd as pkg
    from dxt_lossless_transform_amd import decode, image
    from oracle import oracle_c

    dev = torch.device("cuda:0")
    lib, img = decode._l(), image._l()
    pkg.load()
    w = h = size
    bpr = (w + 3) // 4
    blocks = image.image_blocks(w, h)
    pitch = 4 * w
    pixels = torch.empty(pitch * h, dtype=torch.uint8, device=dev)
    records = torch.empty(64 * (blocks + 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:   # warm up by wall time: the chip ramps its clocks after idling
            for _ in range(4):
                fn()
            torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(steps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps

    out = {}
    for fmt in ("bc1", "bc2", "bc3"):
        bs = BLOCK[fmt]
        settings = {"bc1": pkg.Bc1TransformSettings(), "bc2": pkg.Bc2TransformSettings(), "bc3": pkg.Bc3TransformSettings()}[fmt]
        forward = getattr(pkg, f"transform_{fmt}_with_settings")
        untransform = getattr(lib, f"dxtlt_untransform_{fmt}_with_settings_device")
        decode_blocks = getattr(lib, f"dxtlt_decode_{fmt}_blocks_device")
        for label, total in (("aligned", blocks), ("odd_total", blocks + 1)):
            seed = 0x1A6E0000 + 16 * FMT_ID[fmt] + (total & 1)
            length = total * bs
            x = torch.empty(length, dtype=torch.uint8, device=dev)
            t = torch.empty_like(x)
            pkg.fill_splitmix64(x, seed)
            forward(x, t, settings)
            torch.cuda.synchronize()

            def fused():
                rc = img.dxtlt_untransform_decode_image_device(FMT_ID[fmt], t.data_ptr(), total, 0, w, h, MODE, SA, SC,
                                                               pixels.data_ptr(), pitch, stream)
                assert rc == 0

            def two_calls():
                if fmt == "bc3":
                    rc = untransform(t.data_ptr(), x.data_ptr(), length, MODE, SA, SC, stream)
                else:
                    rc = untransform(t.data_ptr(), x.data_ptr(), length, MODE, SC, stream)
                assert rc == 0
                rc = decode_blocks(x.data_ptr(), length, records.data_ptr(), 64 * total, stream)
                assert rc == 0

            # exactness first: three rows of the fused call's image against the CPU oracle
            pixels.zero_()
            fused()
            torch.cuda.synchronize()
            for y in (1, h // 2 + 2, h - 1):
                by = y // 4
                row_blocks = oracle_c.fill_splitmix64(bpr * bs, seed, by * bpr * bs // 8)
                want = oracle_c.decode_blocks(fmt, row_blocks).reshape(bpr, 4, 4, 4)[:, y % 4].reshape(-1)[:4 * w]
                got = pixels[y * pitch:y * pitch + 4 * w].cpu().numpy()
                assert np.array_equal(got, want), (fmt, label, y)
            # alternate the two variants, twice each; keep the better time of each
            ms_a = ms_b = float("inf")
            for _ in range(2):
                ms_a = min(ms_a, timed(fused))
                ms_b = min(ms_b, timed(two_calls))
            bytes_a = length + 4 * w * h
            bytes_b = 3 * length + 64 * total
            out[f"{fmt}_{label}"] = {"fused_ms": round(ms_a, 4), "fused_peak": round(bytes_a / (ms_a * 1e-3) / PEAK, 4),
                                     "two_calls_ms": round(ms_b, 4), "two_calls_peak": round(bytes_b / (ms_b * 1e-3) / PEAK, 4)}
            del x, t
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_decode_bench.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.size, a.steps)
        return
    runs = []
    for _ in range(a.processes):   # fresh processes, one after the other; this one never opens the device
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--steps", str(a.steps)],
                           stdout=subprocess.PIPE, text=True, check=True)
        runs.append(json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]))
    cells = {}
    for cell in runs[0]:
        c = {}
        for key in runs[0][cell]:
            samples = [r[cell][key] for r in runs]
            c[key] = {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}
        c["fused_is_faster_in_every_process"] = all(r[cell]["fused_ms"] < r[cell]["two_calls_ms"] for r in runs)
        c["speedup_median"] = round(c["two_calls_ms"]["median"] / c["fused_ms"]["median"], 3)
        cells[cell] = c
    result = {"workload": f"{a.size} x {a.size} RGBA8888, default settings, {a.steps} steps per timing, {a.processes} processes",
              "bytes": {"fused": "len + 4 w h", "two_calls": "3 len + 64 blocks"}, "peak_bytes_per_s": PEAK, "cells": cells}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({cell: {"fused_ms": c["fused_ms"]["median"], "two_calls_ms": c["two_calls_ms"]["median"],
                             "fused_peak": c["fused_peak"]["median"], "two_calls_peak": c["two_calls_peak"]["median"]}
                      for cell, c in cells.items()}))


if __name__ == "__main__":
    main()
