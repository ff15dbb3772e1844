#!/usr/bin/env python3
"""A whole BC6H mip chain from a transformed buffer: one dxtlt_untransform_decode_bc6h_images_device call against one single-image
call per level (include/dxtlt_bc6h_image.h; docs/IMAGE_DECODE.md, "Several images of one BC6H buffer").  The method is that of
tools/bc7_image_regions_bench.py.

Per kind of data (every block of class 12, and the every-class mix of tools/bc6h_bench.py, the reserved values included) and per
full chain (256^2: 9 levels, 1024^2: 11, 4096^2: 13, 16384^2: 15), HIP-event times after a warm-up of
  (a) dxtlt_untransform_decode_bc6h_images_device, one call per chain;
  (b) dxtlt_untransform_decode_bc6h_image_device, one call per level, back to back on one stream;
  (c) 16384^2 only: the single-image call for level 0 of the same buffer;
  (d) 16384^2 only: the new call with level 0 as its one region -- (c)'s launch with the region sink, which separates the price
      of the lookup from that of the chain's other levels and its tail-part launch.
(a), (c) and (d) are also stated as a fraction of the 8 TB/s HBM peak on the bytes they must move, 16 blocks + 8 sum(w h).
Before a cell is timed, three rows of every level of (a)'s images are compared with the numpy statement of the decoder
(tests/bc6h_decode_ref.py).  The variants are alternated, twice each, and the better time of each kept.  Every cell is measured in
`--processes` fresh processes, one after the other, each under a time limit of its own; the first failure ends the run.  The
file keeps every sample.

    python tools/bc6h_image_regions_bench.py [--processes 3] [--out profiles/bc6h_image_regions_bench.json]
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
CHAINS = ((256, 9, 2000), (1024, 11, 2000), (4096, 13, 1000), (16384, 15, 100))   # size, levels, steps per timing
CHILD_LIMIT_S = 420


def child():
    """one process: every cell once; prints one JSON line"""
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
    for size, mips, steps in CHAINS:
        regions, total = image.mip_chain(size, size, mips)
        for data in DATA:
            x = torch.empty(total * 16, dtype=torch.uint8, device=dev)
            t = torch.empty_like(x)
            pkg.fill_splitmix64(x, 0x0BC60100 + mips, 0)
            force_classes(torch, x, data)
            bc6h.transform_bc6h(x, t)
            torch.cuda.synchronize()
            # one allocation for all levels, every level on a 256-byte address; a level's pitch is its row
            at, offsets = 0, []
            for _, w, h in regions:
                offsets.append(at)
                at += (8 * w * h + 255) // 256 * 256
            pixels = torch.empty(at, dtype=torch.uint8, device=dev)
            table = (image.ImageRegion * len(regions))()
            for k, (first, w, h) in enumerate(regions):
                table[k] = image.ImageRegion(first, w, h, pixels.data_ptr() + offsets[k], 8 * w)

            def chain_call(count=len(regions)):
                assert img.dxtlt_untransform_decode_bc6h_images_device(t.data_ptr(), total, table, count, stream) == 0

            def level_call(k):
                r = table[k]
                assert img.dxtlt_untransform_decode_bc6h_image_device(t.data_ptr(), total, r.first_block, r.width, r.height, r.pixels,
                                                                      r.pitch, stream) == 0

            def per_level():
                for k in range(len(regions)):
                    level_call(k)

            # exactness first: three rows of every level of the chain call's images against the numpy statement
            pixels.zero_()
            chain_call()
            torch.cuda.synchronize()
            for k, (first, w, h) in enumerate(regions):
                bpr = (w + 3) // 4
                for y in sorted({min(1, h - 1), min(h // 2 + 2, h - 1), h - 1}):
                    src = 16 * (first + (y // 4) * bpr)
                    row = x[src:src + 16 * bpr].cpu().numpy()
                    want = ref.image_bytes(ref.decode_blocks(row), w, min(4, h - y // 4 * 4))[y % 4]
                    got = pixels[offsets[k] + y * 8 * w:offsets[k] + (y + 1) * 8 * w].cpu().numpy()
                    assert np.array_equal(got, want), (data, size, k, y)
            del x
            variants = {"chain": chain_call, "per_level": per_level}
            if size == 16384:
                variants["level0"] = lambda: level_call(0)
                variants["level0_region"] = lambda: chain_call(1)
            ms = {name: float("inf") for name in variants}
            for _ in range(2):   # alternate the variants, twice each; keep the better time of each
                for name, fn in variants.items():
                    ms[name] = min(ms[name], timed(fn, steps))
            cell = {f"{name}_ms": round(v, 5) for name, v in ms.items()}
            bytes_chain = 16 * total + 8 * sum(w * h for _, w, h in regions)
            cell["chain_peak"] = round(bytes_chain / (ms["chain"] * 1e-3) / PEAK, 4)
            if size == 16384:
                _, w, h = regions[0]
                for name in ("level0", "level0_region"):
                    cell[name + "_peak"] = round((16 * image.image_blocks(w, h) + 8 * w * h) / (ms[name] * 1e-3) / PEAK, 4)
            out[f"{data}_{size}"] = cell
            del t, pixels
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc6h_image_regions_bench.json"))
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
        # the cell's spread: the wider range of the two variants under comparison over the processes, in ms
        spread = max(c[k]["max"] - c[k]["min"] for k in ("chain_ms", "per_level_ms"))
        c["spread_ms"] = round(spread, 5)
        c["speedup_median"] = round(c["per_level_ms"]["median"] / c["chain_ms"]["median"], 3)
        c["chain_faster_than_per_level_by_more_than_the_spread_in_every_process"] = all(
            r[cell]["per_level_ms"] - r[cell]["chain_ms"] > spread for r in runs)
        c["chain_not_slower_than_per_level_by_more_than_the_spread"] = all(
            r[cell]["chain_ms"] - r[cell]["per_level_ms"] <= spread for r in runs)
        if "level0_peak" in c:
            c["chain_peak_minus_level0_peak_per_process"] = [round(r[cell]["chain_peak"] - r[cell]["level0_peak"], 4) for r in runs]
            c["level0_region_peak_minus_level0_peak_per_process"] = [round(r[cell]["level0_region_peak"] - r[cell]["level0_peak"], 4)
                                                                     for r in runs]
        cells[cell] = c
    small = [c for name, c in cells.items() if name.endswith(("_256", "_1024"))]
    large = [c for name, c in cells.items() if name.endswith(("_4096", "_16384"))]
    result = {"workload": f"full BC6H mip chains, {a.processes} processes; (size, levels, steps per timing) = {list(CHAINS)}; data = {list(DATA)}",
              "variants": {"chain": "one dxtlt_untransform_decode_bc6h_images_device call",
                           "per_level": "one dxtlt_untransform_decode_bc6h_image_device call per level",
                           "level0": "the single-image fused call for level 0 alone",
                           "level0_region": "the new call with level 0 as its one region"},
              "bytes": "16 * blocks + 8 * sum(w h)", "peak_bytes_per_s": PEAK,
              "expectations": {
                  "chain faster than per_level in every process of the 256 and 1024 cells by more than the cell's spread":
                      all(c["chain_faster_than_per_level_by_more_than_the_spread_in_every_process"] for c in small),
                  "chain not slower than per_level beyond the spread at 4096 and 16384":
                      all(c["chain_not_slower_than_per_level_by_more_than_the_spread"] for c in large)},
              "cells": cells}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({cell: {k: (v["median"] if isinstance(v, dict) else v) for k, v in c.items()} for cell, c in cells.items()}))


if __name__ == "__main__":
    main()
