#!/usr/bin/env python3
"""The images of many BC6H transformed buffers: one dxtlt_untransform_decode_bc6h_images_batch_device call against one
dxtlt_untransform_decode_bc6h_images_device call per buffer (include/dxtlt_bc6h_image.h; docs/IMAGE_DECODE.md, "Many BC6H buffers
in one call").  The method is that of tools/bc7_image_batch_bench.py.

Per kind of data (every block of class 12, and the every-class mix of tools/bc6h_bench.py, the reserved values included) and per
cell (8000 x 256^2, 1024 x 1024^2, 64 x 4096^2 full mip chains, every buffer and every image on a 256-byte address, pitch =
8 * width), HIP-event times after a warm-up of
  (a) batch      dxtlt_untransform_decode_bc6h_images_batch_device, one call per cell;
  (b) per_item   dxtlt_untransform_decode_bc6h_images_device, one call per item, back to back on one stream.
(a) is also stated as a fraction of the 8 TB/s HBM peak on the bytes it must move, sum over the items of 16 * blocks +
8 * sum(w h); (b) too, so that the 4096^2 cell can stand beside the region call's fraction for one such buffer
(profiles/bc6h_image_regions_bench.json).  Before a cell is timed, three rows of every level of four items' images are compared
with the numpy statement of the decoder (tests/bc6h_decode_ref.py).  The variants are alternated, twice each, and the better time
of each kept.  Every cell is measured in `--processes` fresh processes, one after the other, each under a time limit of its own;
the first failure ends the run.  The file keeps every sample.

    python tools/bc6h_image_batch_bench.py [--processes 3] [--out profiles/bc6h_image_batch_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK = 8e12
DATA = ("class12", "mixed")
# items, size, levels, steps per timing of (a), of (b)
CELLS = ((8000, 256, 9, 20, 3), (1024, 1024, 11, 20, 6), (64, 4096, 13, 20, 20))
CHILD_LIMIT_S = 300


def child():
    """one process: every cell once; prints one JSON line"""
    import ctypes as C
    import time

    import numpy as np
    import torch

    import dxt_lossless_transform_amd as pkg
    from bc6h_image_bench import force_classes
    from dxt_lossless_transform_amd import bc6h, image

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bc6h_decode_ref as ref

    dev = torch.device("cuda:0")
    pkg.load()
    img = image._l()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn, steps):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:   # warm up by wall time: the chip ramps its clocks after idling
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
    for count, size, mips, steps_batch, steps_loop in CELLS:
        regions, total = image.mip_chain(size, size, mips)
        for data in DATA:
            stride = (total * 16 + 255) // 256 * 256            # every buffer on a 256-byte address
            x = torch.empty(count * stride, dtype=torch.uint8, device=dev)
            t = torch.empty_like(x)
            pkg.fill_splitmix64(x, 0x0BC60200 + mips, 0)
            force_classes(torch, x, data)
            for i in range(count):
                bc6h.transform_bc6h(x[i * stride:i * stride + total * 16], t[i * stride:i * stride + total * 16])
            torch.cuda.synchronize()
            # one allocation for all images, every level on a 256-byte address; a level's pitch is its row
            at, offsets = 0, []
            for _, w, h in regions:
                offsets.append(at)
                at += (8 * w * h + 255) // 256 * 256
            pixels = torch.empty(count * at, dtype=torch.uint8, device=dev)
            tables, items = [], (image.Bc6hImageBatchItem * count)()
            for i in range(count):
                table = (image.ImageRegion * len(regions))()
                for k, (first, w, h) in enumerate(regions):
                    table[k] = image.ImageRegion(first, w, h, pixels.data_ptr() + i * at + offsets[k], 8 * w)
                tables.append(table)
                items[i] = image.Bc6hImageBatchItem(t.data_ptr() + i * stride, total, C.cast(table, C.c_void_p), len(regions), 0)

            def batch_call():
                assert img.dxtlt_untransform_decode_bc6h_images_batch_device(items, count, stream) == 0

            def per_item():
                for i in range(count):
                    assert img.dxtlt_untransform_decode_bc6h_images_device(t.data_ptr() + i * stride, total, tables[i], len(regions), stream) == 0

            # exactness first: three rows of every level of four items' images from the batch call against the numpy statement
            pixels.zero_()
            batch_call()
            torch.cuda.synchronize()
            for i in sorted({0, 1, count // 2, count - 1}):
                for k, (first, w, h) in enumerate(regions):
                    bpr = (w + 3) // 4
                    for y in sorted({min(1, h - 1), min(h // 2 + 2, h - 1), h - 1}):
                        src = i * stride + 16 * (first + (y // 4) * bpr)
                        row = x[src:src + 16 * bpr].cpu().numpy()
                        want = ref.image_bytes(ref.decode_blocks(row), w, min(4, h - y // 4 * 4))[y % 4]
                        a0 = i * at + offsets[k] + y * 8 * w
                        got = pixels[a0:a0 + 8 * w].cpu().numpy()
                        assert np.array_equal(got, want), (data, size, i, k, y)
            del x
            variants = {"batch": (batch_call, steps_batch), "per_item": (per_item, steps_loop)}
            ms = {name: float("inf") for name in variants}
            for _ in range(2):   # alternate the variants, twice each; keep the better time of each
                for name, (fn, steps) in variants.items():
                    ms[name] = min(ms[name], timed(fn, steps))
            cell = {f"{name}_ms": round(v, 5) for name, v in ms.items()}
            moved = count * (total * 16 + 8 * sum(w * h for _, w, h in regions))
            for name in variants:
                cell[f"{name}_peak"] = round(moved / (ms[name] * 1e-3) / PEAK, 4)
            out[f"{data}_{count}x{size}"] = cell
            del t, pixels, tables, items
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc6h_image_batch_bench.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child()
        return
    runs = []
    for k in range(a.processes):   # fresh processes, one after the other; this one never opens the device
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child"],
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:      # the first failure ends the run: nothing more is started on the device
            sys.exit(f"a measuring process ended with status {p.returncode}")
        runs.append(json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]))
        print(f"process {k + 1} of {a.processes} done", file=sys.stderr, flush=True)
    cells = {}
    for cell in runs[0]:
        c = {}
        for key in runs[0][cell]:
            samples = [r[cell][key] for r in runs]
            c[key] = {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}
        # the cell's spread: the wider range of the two variants over the processes, in ms
        spread = max(c[k]["max"] - c[k]["min"] for k in ("batch_ms", "per_item_ms"))
        c["spread_ms"] = round(spread, 5)
        c["speedup_over_per_item_median"] = round(c["per_item_ms"]["median"] / c["batch_ms"]["median"], 3)
        c["batch_faster_than_per_item_by_more_than_the_spread_in_every_process"] = all(
            r[cell]["per_item_ms"] - r[cell]["batch_ms"] > spread for r in runs)
        c["batch_not_slower_than_per_item_by_more_than_the_spread"] = all(
            r[cell]["batch_ms"] - r[cell]["per_item_ms"] <= spread for r in runs)
        cells[cell] = c
    small = [c for name, c in cells.items() if name.endswith(("x256", "x1024"))]
    large = [c for name, c in cells.items() if name.endswith("x4096")]
    result = {"workload": f"full BC6H mip chains, {a.processes} processes; (items, size, levels, steps per timing of the batch call, of "
                          f"the loop) = {list(CELLS)}; data = {list(DATA)}",
              "variants": {"batch": "one dxtlt_untransform_decode_bc6h_images_batch_device call",
                           "per_item": "one dxtlt_untransform_decode_bc6h_images_device call per item"},
              "bytes": "sum over the items of 16 * blocks + 8 * sum(w h)", "peak_bytes_per_s": PEAK,
              "expectations": {
                  "batch faster than per_item in every process of the 8000 x 256 and 1024 x 1024 cells by more than the cell's spread":
                      all(c["batch_faster_than_per_item_by_more_than_the_spread_in_every_process"] for c in small),
                  "batch not slower than per_item beyond the spread at 64 x 4096":
                      all(c["batch_not_slower_than_per_item_by_more_than_the_spread"] for c in large)},
              "cells": cells}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({cell: {k: (v["median"] if isinstance(v, dict) else v) for k, v in c.items()} for cell, c in cells.items()}))


if __name__ == "__main__":
    main()
