#!/usr/bin/env python3
"""Fused BC7 untransform + image decode (include/dxtlt_bc7_image.h) against the two calls it replaces, on one MI355X.

A 16384 x 16384 image (16 777 216 blocks).  Cells: three kinds of data -- every block of mode 6, and the uniform and the skewed
mode mix of `bench.py --format bc7` -- each with the image's blocks alone in the transformed buffer (`image`) and with a total
that leaves a tail part and a first_block in mid-granule (`offset`).  Variants, HIP-event times after a warm-up, alternated:
  (a) dxtlt_untransform_decode_bc7_image_device                                  -- must move len + 4 w h = 80 bytes per block
  (b) dxtlt_untransform_bc7_device into scratch + dxtlt_decode_bc7_image_device  -- must move 3 len + 4 w h = 112 bytes per block
  (c) dxtlt_untransform_decode_image_device, BC3, on an image of the same size in the same process: context
and the fraction of the 8 TB/s HBM peak each reaches on its own bytes.  Before a cell is timed, three rows of (a)'s image are
compared with the CPU statement of the decoder (tests/bc7_decode_ref.py).  Every cell is measured in `--processes` fresh
processes, each under a time limit of its own; the first failure ends the run; the file keeps every sample.

The expectation under test: (a) is faster than (b) in every process of every cell by more than the cell's spread -- the larger
of the two variants' max - min over its processes.

    python tools/bc7_image_bench.py [--size 16384] [--steps 200] [--processes 3] [--out profiles/bc7_image_bench.json]
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
GRANULE = 1024
DATA = ("mode6", "uniform", "skewed")
LAYOUTS = ("image", "offset")
CHILD_LIMIT_S = 240
# The forms of the fused kernel that were built, measured with this tool's child processes (one process per figure, 200 calls per
# timing, the same box) from builds that carried them side by side behind a switch; only the last one is in the tree
# (csrc/bc7_image_kernels.hip, Bc7PixelSink).  fused_ms per cell.
AB = {
    "how": "single child processes of this tool, --steps 200, all forms in one build behind a switch, run one after the other",
    "block_order_decode_behind_the_unsort_19_KiB_lds": {"mode6_image": 0.2382, "uniform_image": 1.4307, "skewed_image": 1.0575, "skewed_offset": 1.0566},
    "staged_sorted_decode_4_rows_per_part_64_KiB_lds": {"mode6_image": 0.2895, "uniform_image": 0.4759, "skewed_image": 0.4522, "skewed_offset": 0.4575},
    "staged_sorted_decode_1_row_per_part_19_KiB_lds": {"mode6_image": 0.2489, "uniform_image": 0.4121, "skewed_image": 0.3667, "skewed_offset": 0.3686},
    "staged_sorted_decode_2_rows_per_part_32_KiB_lds_kept": {"mode6_image": 0.2306, "uniform_image": 0.4012, "skewed_image": 0.3550, "skewed_offset": 0.3576},
    "two_calls_in_the_same_processes": {"mode6_image": 0.2955, "uniform_image": 1.4209, "skewed_image": 1.0308, "skewed_offset": 1.0354},
}


def force_modes(torch, x, data):
    """mode-mixed BC7 data in place, as bench.py's bc7_force_modes_device: for mode m the low m + 1 bits of byte 0 become 1 << m"""
    b = x.view(-1, 16)
    for lo in range(0, b.shape[0], 1 << 24):
        v = b[lo:lo + (1 << 24)]
        r = v[:, 15].to(torch.int32)
        if data == "mode6":
            m = torch.full_like(r, 6)
        elif data == "uniform":
            m = r & 7
        else:
            m = torch.where(r < 140, 6, torch.where(r < 200, 1, torch.where(r < 230, 3, r & 7))).to(torch.int32)
        low = ((2 << m) - 1).to(torch.uint8)
        v[:, 0] = (v[:, 0] & ~low) | (1 << m).to(torch.uint8)
        del r, m, low


def child(size, steps, data, layout):
    """one process: one cell; prints one JSON line"""
    import time

    import numpy as np
    import torch

    import dxt_lossless_transform_amd as pkg
    from dxt_lossless_transform_amd import bc7, image

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bc7_decode_ref as ref

    dev = torch.device("cuda:0")
    pkg.load()
    img = image._l()
    w = h = size
    bpr = (w + 3) // 4
    blocks = image.image_blocks(w, h)
    first, total = (0, blocks) if layout == "image" else (3 * GRANULE + 500, 3 * GRANULE + 500 + blocks + 777)
    assert layout == "image" or (first % GRANULE != 0 and total % GRANULE != 0)
    pitch = 4 * w
    pixels = torch.empty(pitch * h, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    length = 16 * total
    x = torch.empty(length, dtype=torch.uint8, device=dev)
    t = torch.empty_like(x)
    scratch = torch.empty_like(x)
    pkg.fill_splitmix64(x, 0x0BC70004, 0)
    force_modes(torch, x, data)
    bc7.transform_bc7(x, t)
    # (c): BC3 of the same image, default settings
    x3 = torch.empty(16 * blocks, dtype=torch.uint8, device=dev)
    t3 = torch.empty_like(x3)
    pkg.fill_splitmix64(x3, 0x1A6E0030, 0)
    pkg.transform_bc3_with_settings(x3, t3, pkg.Bc3TransformSettings())
    del x3
    torch.cuda.synchronize()
    untransform = bc7._l().dxtlt_untransform_bc7_device

    def fused():
        assert img.dxtlt_untransform_decode_bc7_image_device(t.data_ptr(), total, first, w, h, pixels.data_ptr(), pitch, stream) == 0

    def two_calls():
        assert untransform(t.data_ptr(), scratch.data_ptr(), length, None, 0, stream) == 0
        assert img.dxtlt_decode_bc7_image_device(scratch.data_ptr() + 16 * first, w, h, pixels.data_ptr(), pitch, stream) == 0

    def bc3_fused():
        assert img.dxtlt_untransform_decode_image_device(3, t3.data_ptr(), blocks, 0, w, h, 1, True, True, pixels.data_ptr(), pitch, stream) == 0

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

    # exactness first: three rows of both BC7 variants' images against the CPU statement
    for variant in (fused, two_calls):
        pixels.zero_()
        variant()
        torch.cuda.synchronize()
        for y in (1, h // 2 + 2, h - 1):
            at = 16 * (first + (y // 4) * bpr)
            row = x[at:at + 16 * bpr].cpu().numpy()
            want = ref.decode_blocks(row).reshape(bpr, 4, 4, 4)[:, y % 4].reshape(-1)[:4 * w]
            got = pixels[y * pitch:y * pitch + 4 * w].cpu().numpy()
            assert np.array_equal(got, want), (variant.__name__, data, layout, y)
    ms = {"fused": float("inf"), "two_calls": float("inf"), "bc3_fused": float("inf")}
    for _ in range(2):   # alternate the variants, twice each; keep the better time of each
        for name, fn in (("fused", fused), ("two_calls", two_calls), ("bc3_fused", bc3_fused)):
            ms[name] = min(ms[name], timed(fn))
    moved = {"fused": length + 4 * w * h, "two_calls": 3 * length + 4 * w * h, "bc3_fused": 16 * blocks + 4 * w * h}
    out = {}
    for name in ms:
        out[name + "_ms"] = round(ms[name], 4)
        out[name + "_peak"] = round(moved[name] / (ms[name] * 1e-3) / PEAK, 4)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc7_image_bench.json"))
    ap.add_argument("--child", nargs=2, metavar=("DATA", "LAYOUT"))
    a = ap.parse_args()
    if a.child:
        child(a.size, a.steps, a.child[0], a.child[1])
        return
    cells = {}
    for data in DATA:
        for layout in LAYOUTS:
            runs = []
            for _ in range(a.processes):   # fresh processes, one after the other; this one never opens the device
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", data, layout, "--size", str(a.size), "--steps",
                                    str(a.steps)], stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT_S)
                if p.returncode != 0:   # the first failure ends the run
                    sys.exit(f"cell {data}_{layout}: a child process ended with status {p.returncode}")
                runs.append(json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]))
            c = {}
            for key in runs[0]:
                samples = [r[key] for r in runs]
                c[key] = {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}
            spread = max(c["fused_ms"]["max"] - c["fused_ms"]["min"], c["two_calls_ms"]["max"] - c["two_calls_ms"]["min"])
            c["spread_ms"] = round(spread, 4)
            c["fused_faster_than_two_calls_by_more_than_the_spread_in_every_process"] = all(
                r["two_calls_ms"] - r["fused_ms"] > spread for r in runs)
            c["two_calls_over_fused_median"] = round(c["two_calls_ms"]["median"] / c["fused_ms"]["median"], 3)
            cells[f"{data}_{layout}"] = c
            print(f"{data}_{layout}", json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in c.items()}), flush=True)
    result = {"workload": f"{a.size} x {a.size} RGBA8888 from BC7, {a.steps} steps per timing, {a.processes} processes per cell",
              "bytes_per_block": {"fused": 80, "two_calls": 112, "bc3_fused": 80}, "peak_bytes_per_s": PEAK,
              "layouts": {"image": "total_blocks = the image's blocks, first_block = 0",
                          "offset": "first_block = 3572 (mid-granule), total_blocks = first_block + image blocks + 777 (a tail part of 253)"},
              "expectation": "fused faster than two_calls in every process of every cell by more than the cell's spread",
              "expectation_met": all(c["fused_faster_than_two_calls_by_more_than_the_spread_in_every_process"] for c in cells.values()),
              "ab": AB,
              "cells": cells}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
