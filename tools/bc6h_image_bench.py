#!/usr/bin/env python3
"""Fused BC6H untransform + image decode (include/dxtlt_bc6h_image.h) against the two calls it replaces, on one MI355X.

A 16384 x 16384 RGBA16F image (16 777 216 blocks, 2 GiB of pixels).  Cells: two kinds of data -- every block of class 12, and
the every-class mix of tools/bc6h_bench.py (the reserved values included) -- each with the image's blocks alone in the
transformed buffer (`image`) and with a total that leaves a tail part and a first_block in mid-granule (`offset`).  Variants,
HIP-event times after a warm-up, alternated:
  (a) dxtlt_untransform_decode_bc6h_image_device                                   -- must move len + 8 w h = 144 bytes per block
  (b) dxtlt_untransform_bc6h_device into scratch + dxtlt_decode_bc6h_image_device  -- must move 3 len + 8 w h = 176 bytes per block
  (c) dxtlt_untransform_decode_bc7_image_device on an image of the same pixel count in the same process: context (80 bytes)
and the fraction of the 8 TB/s HBM peak each reaches on its own bytes.  Before a cell is timed, three rows of (a)'s and (b)'s
image are compared with the CPU statement of the decoder (tests/bc6h_decode_ref.py).  Every cell is measured in `--processes`
fresh processes, each under a time limit of its own; the first failure ends the run; the file keeps every sample.

The expectation under test: (a) is faster than (b) in every process of every cell by more than the cell's spread -- the larger
of the two variants' max - min over its processes.

    python tools/bc6h_image_bench.py [--size 16384] [--steps 100] [--processes 3] [--out profiles/bc6h_image_bench.json]
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
DATA = ("class12", "mixed")
LAYOUTS = ("image", "offset")
CHILD_LIMIT_S = 240
# The forms of the fused kernel that were built, measured with this tool's child processes (one process per figure, 100 calls per
# timing, the same box, one after the other) from side builds that carried them behind compile-time switches; only the last one is in
# the tree (csrc/bc6h_image_sinks.h, Bc6hPixelSink).  fused_ms per cell.  "plain_decoder_stores": two_calls_ms, the fused kernel the
# same in both builds.
AB = {
    "how": "single child processes of this tool, --steps 100, one side build per form, run one after the other; the kept form first and last",
    "form_1_own_block_row_two_sc1_nt_stores_per_lane_256x4_1_row_per_part_32_KiB": {"class12_image": 1.9873, "mixed_image": 1.9926, "mixed_offset": 2.0473},
    "form_1_2_rows_per_part_64_KiB": {"class12_image": 2.0312, "mixed_image": 2.0223, "mixed_offset": 2.0647},
    "form_1_512_lanes_x_2_blocks": {"class12_image": 1.9592, "mixed_image": 1.9576, "mixed_offset": 2.0289},
    "form_2_pieces_l_and_64_plus_l_512_lanes_x_2_blocks": {"class12_image": 0.5156, "mixed_image": 0.5128, "mixed_offset": 0.5140},
    "form_2_pieces_l_and_64_plus_l_256x4_1_row_per_part_32_KiB_kept": {"class12_image": [0.4940, 0.4925, 0.4936], "mixed_image": [0.5446, 0.5421, 0.5421],
                                                                       "mixed_offset": [0.5468, 0.5426, 0.5432]},
    "plain_decoder_stores": {"sc1_nt_when_aligned_two_calls_ms": {"class12_image": 1.9807, "mixed_image": 2.0544, "mixed_offset": 2.0548},
                             "plain_kept_two_calls_ms": {"class12_image": 0.5526, "mixed_image": 0.8952, "mixed_offset": 0.9010}},
    "not_built": "RGB staged at 24 bytes per row with alpha added at the store; form 2 with two rows per part; decoding from the record",
}


def force_classes(torch, x, data):
    """class-mixed BC6H data in place, as tools/bc6h_bench.py make(): class byte 15 % 15 (14 = a reserved value), or class 12"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bc6h_ref as R

    b = x.view(-1, 16)
    codes = torch.tensor(list(R.MODE_BITS) + [19], dtype=torch.uint8, device=x.device)
    for lo in range(0, b.shape[0], 1 << 24):
        v = b[lo:lo + (1 << 24)]
        k = (v[:, 15].to(torch.int64) % 15) if data == "mixed" else torch.full((v.shape[0],), 12, dtype=torch.int64, device=x.device)
        mb = torch.where(k <= 1, 3, 0x1F).to(torch.uint8)
        v[:, 0] = (v[:, 0] & ~mb) | codes[k]
        del k, mb


def child(size, steps, data, layout):
    """one process: one cell; prints one JSON line"""
    import time

    import numpy as np
    import torch

    import dxt_lossless_transform_amd as pkg
    from dxt_lossless_transform_amd import bc6h, bc7, image

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bc6h_decode_ref as ref

    dev = torch.device("cuda:0")
    pkg.load()
    img = image._l()
    w = h = size
    bpr = (w + 3) // 4
    blocks = image.image_blocks(w, h)
    first, total = (0, blocks) if layout == "image" else (3 * GRANULE + 500, 3 * GRANULE + 500 + blocks + 777)
    assert layout == "image" or (first % GRANULE != 0 and total % GRANULE != 0)
    pitch = 8 * w
    pixels = torch.empty(pitch * h, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    length = 16 * total
    x = torch.empty(length, dtype=torch.uint8, device=dev)
    t = torch.empty_like(x)
    scratch = torch.empty_like(x)
    pkg.fill_splitmix64(x, 0x0BC60004, 0)
    force_classes(torch, x, data)
    bc6h.transform_bc6h(x, t)
    # (c): BC7 of the same pixel count, the uniform mode mix of tools/bc7_image_bench.py
    x7 = torch.empty(16 * blocks, dtype=torch.uint8, device=dev)
    t7 = torch.empty_like(x7)
    pkg.fill_splitmix64(x7, 0x0BC70004, 0)
    b7 = x7.view(-1, 16)
    m = (b7[:, 15] & 7).to(torch.int32)
    low = ((2 << m) - 1).to(torch.uint8)
    b7[:, 0] = (b7[:, 0] & ~low) | (1 << m).to(torch.uint8)
    del m, low
    bc7.transform_bc7(x7, t7)
    del x7
    torch.cuda.synchronize()
    untransform = bc6h._l().dxtlt_untransform_bc6h_device

    def fused():
        assert img.dxtlt_untransform_decode_bc6h_image_device(t.data_ptr(), total, first, w, h, pixels.data_ptr(), pitch, stream) == 0

    def two_calls():
        assert untransform(t.data_ptr(), scratch.data_ptr(), length, stream) == 0
        assert img.dxtlt_decode_bc6h_image_device(scratch.data_ptr() + 16 * first, w, h, pixels.data_ptr(), pitch, stream) == 0

    def bc7_fused():
        assert img.dxtlt_untransform_decode_bc7_image_device(t7.data_ptr(), blocks, 0, w, h, pixels.data_ptr(), 4 * w, stream) == 0

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

    # exactness first: three rows of both BC6H variants' images against the CPU statement
    for variant in (fused, two_calls):
        pixels.zero_()
        variant()
        torch.cuda.synchronize()
        for y in (1, h // 2 + 2, h - 1):
            at = 16 * (first + (y // 4) * bpr)
            row = x[at:at + 16 * bpr].cpu().numpy()
            want = ref.image_bytes(ref.decode_blocks(row), w, 4)[y % 4]
            got = pixels[y * pitch:y * pitch + 8 * w].cpu().numpy()
            assert np.array_equal(got, want), (variant.__name__, data, layout, y)
    ms = {"fused": float("inf"), "two_calls": float("inf"), "bc7_fused": float("inf")}
    for _ in range(2):   # alternate the variants, twice each; keep the better time of each
        for name, fn in (("fused", fused), ("two_calls", two_calls), ("bc7_fused", bc7_fused)):
            ms[name] = min(ms[name], timed(fn))
    moved = {"fused": length + 8 * w * h, "two_calls": 3 * length + 8 * w * h, "bc7_fused": 16 * blocks + 4 * w * h}
    out = {}
    for name in ms:
        out[name + "_ms"] = round(ms[name], 4)
        out[name + "_peak"] = round(moved[name] / (ms[name] * 1e-3) / PEAK, 4)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc6h_image_bench.json"))
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
    result = {"workload": f"{a.size} x {a.size} RGBA16F from BC6H, {a.steps} steps per timing, {a.processes} processes per cell",
              "bytes_per_block": {"fused": 144, "two_calls": 176, "bc7_fused": 80}, "peak_bytes_per_s": PEAK,
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
