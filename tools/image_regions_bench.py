#!/usr/bin/env python3
"""A whole mip chain from a transformed buffer: one dxtlt_untransform_decode_images_device call against one single-image call
per level (include/dxtlt_image.h; docs/IMAGE_DECODE.md, "Several images of one buffer").

Per format (BC1, BC3, BC4, default settings) and per full chain (256^2: 9 levels, 1024^2: 11, 4096^2: 13, 16384^2: 15 -- every
total is odd, so every plan is shifted tiles), HIP-event times after a warm-up of
  (a) dxtlt_untransform_decode_images_device, one call per chain;
  (b) dxtlt_untransform_decode_image_device / ..._channel_image_device, one call per level, back to back on one stream;
  (c) 16384^2 only: the single-image call for level 0 of the same buffer.
(a) and (c) are also stated as a fraction of the 8 TB/s HBM peak on the bytes they must move, len_covered + bpp * sum(w h).
Before a cell is timed, three rows of every level of (a)'s images are compared with the CPU oracle.  The variants are alternated,
twice each, and the better time of each kept.  Every cell is measured in `--processes` fresh processes, one after the other,
each under a time limit of its own; the first failure ends the run.  The file keeps every sample.

    python tools/image_regions_bench.py [--processes 3] [--out profiles/image_regions_bench.json]
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
FMT_ID = {"bc1": 1, "bc3": 3, "bc4": 4}
BLOCK = {"bc1": 8, "bc3": 16, "bc4": 8}
BPP = {"bc1": 4, "bc3": 4, "bc4": 1}
SETTINGS = {"bc1": (1, False, True), "bc3": (1, True, True), "bc4": (0, False, False)}   # the settings types' defaults
CHAINS = ((256, 9, 4000), (1024, 11, 3000), (4096, 13, 1500), (16384, 15, 300))           # size, levels, steps per timing
CHILD_LIMIT_S = 420


def expected_row(oracle_c, np, fmt, seed, first, width, y):
    """row y of the image whose blocks start at block `first` of the splitmix64 stream `seed`"""
    bs, bpr = BLOCK[fmt], (width + 3) // 4
    blocks = oracle_c.fill_splitmix64(bpr * bs, seed, (first + (y // 4) * bpr) * bs // 8)
    if fmt == "bc4":   # a BC4 block is the alpha half of a BC3 block
        bc3 = np.zeros((bpr, 16), dtype=np.uint8)
        bc3[:, :8] = blocks.reshape(bpr, 8)
        px = oracle_c.decode_blocks("bc3", bc3.reshape(-1)).reshape(bpr, 4, 4, 4)[:, y % 4, :, 3]
        return px.reshape(-1)[:width]
    return oracle_c.decode_blocks(fmt, blocks).reshape(bpr, 4, 4, 4)[:, y % 4].reshape(-1)[:4 * width]


def child():
    """one process: every cell once; prints one JSON line"""
    import ctypes as C
    import time

    import numpy as np
    import torch

    import dxt_lossless_transform_amd as pkg
    from dxt_lossless_transform_amd import _lib, image
    from oracle import oracle_c

    dev = torch.device("cuda:0")
    core, img = _lib.load(), image._l()
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
        assert total % 2 == 1
        for fmt in ("bc1", "bc3", "bc4"):
            bs, bpp, (mode, sa, sc) = BLOCK[fmt], BPP[fmt], SETTINGS[fmt]
            seed = 0x5E610000 + 16 * FMT_ID[fmt] + mips
            x = torch.empty(total * bs, dtype=torch.uint8, device=dev)
            t = torch.empty_like(x)
            pkg.fill_splitmix64(x, seed)
            assert core.dxtlt_transform_range_device(FMT_ID[fmt], False, x.data_ptr(), t.data_ptr(), total, 0, total, mode, sa, sc,
                                                     stream) == 0
            torch.cuda.synchronize()
            del x
            # one allocation for all levels, every level on a 256-byte address; a level's pitch is its row
            at, offsets = 0, []
            for _, w, h in regions:
                offsets.append(at)
                at += (bpp * w * h + 255) // 256 * 256
            pixels = torch.empty(at, dtype=torch.uint8, device=dev)
            table = (image.ImageRegion * len(regions))()
            for k, (first, w, h) in enumerate(regions):
                table[k] = image.ImageRegion(first, w, h, pixels.data_ptr() + offsets[k], bpp * w)

            def chain_call():
                rc = img.dxtlt_untransform_decode_images_device(FMT_ID[fmt], t.data_ptr(), total, table, len(regions), mode, sa, sc, stream)
                assert rc == 0

            def level_call(k):
                r = table[k]
                if fmt == "bc4":
                    rc = img.dxtlt_untransform_decode_channel_image_device(FMT_ID[fmt], t.data_ptr(), total, r.first_block, r.width,
                                                                           r.height, sa, r.pixels, r.pitch, stream)
                else:
                    rc = img.dxtlt_untransform_decode_image_device(FMT_ID[fmt], t.data_ptr(), total, r.first_block, r.width, r.height,
                                                                   mode, sa, sc, r.pixels, r.pitch, stream)
                assert rc == 0

            def per_level():
                for k in range(len(regions)):
                    level_call(k)

            # exactness first: three rows of every level of the chain call's images against the CPU oracle
            pixels.zero_()
            chain_call()
            torch.cuda.synchronize()
            for k, (first, w, h) in enumerate(regions):
                for y in sorted({min(1, h - 1), min(h // 2 + 2, h - 1), h - 1}):
                    got = pixels[offsets[k] + y * bpp * w:offsets[k] + (y + 1) * bpp * w].cpu().numpy()
                    assert np.array_equal(got, expected_row(oracle_c, np, fmt, seed, first, w, y)), (fmt, size, k, y)
            variants = {"chain": chain_call, "per_level": per_level}
            if size == 16384:
                variants["level0"] = lambda: level_call(0)
            ms = {name: float("inf") for name in variants}
            for _ in range(2):   # alternate the variants, twice each; keep the better time of each
                for name, fn in variants.items():
                    ms[name] = min(ms[name], timed(fn, steps))
            cell = {f"{name}_ms": round(v, 5) for name, v in ms.items()}
            bytes_chain = total * bs + bpp * sum(w * h for _, w, h in regions)
            cell["chain_peak"] = round(bytes_chain / (ms["chain"] * 1e-3) / PEAK, 4)
            if size == 16384:
                first, w, h = regions[0]
                cell["level0_peak"] = round((image.image_blocks(w, h) * bs + bpp * w * h) / (ms["level0"] * 1e-3) / PEAK, 4)
            out[f"{fmt}_{size}"] = cell
            del t, pixels
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_regions_bench.json"))
    ap.add_argument("--note", default="", help="a line kept in the file, e.g. which lookup the library was built with")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child()
        return
    runs = []
    for _ in range(a.processes):   # fresh processes, one after the other; this one never opens the device
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child"],
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:      # the first failure ends the run: nothing more is started on the device
            sys.exit(f"a measuring process ended with status {p.returncode}")
        runs.append(json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]))
    cells = {}
    for cell in runs[0]:
        c = {}
        for key in runs[0][cell]:
            samples = [r[cell][key] for r in runs]
            c[key] = {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}
        # the cell's spread: the widest range any of its variants shows over the processes, in ms
        spread = max(c[k]["max"] - c[k]["min"] for k in c if k.endswith("_ms"))
        c["spread_ms"] = round(spread, 5)
        c["speedup_median"] = round(c["per_level_ms"]["median"] / c["chain_ms"]["median"], 3)
        c["chain_faster_than_per_level_by_more_than_the_spread_in_every_process"] = all(
            r[cell]["per_level_ms"] - r[cell]["chain_ms"] > spread for r in runs)
        c["chain_not_slower_than_per_level_by_more_than_the_spread"] = all(
            r[cell]["chain_ms"] - r[cell]["per_level_ms"] <= spread for r in runs)
        if "level0_peak" in c:
            c["chain_peak_minus_level0_peak_per_process"] = [round(r[cell]["chain_peak"] - r[cell]["level0_peak"], 4) for r in runs]
        cells[cell] = c
    result = {"workload": f"full mip chains, default settings, {a.processes} processes; (size, levels, steps per timing) = {list(CHAINS)}",
              "variants": {"chain": "one dxtlt_untransform_decode_images_device call", "per_level": "one single-image fused call per level",
                           "level0": "the single-image fused call for level 0 alone"},
              "bytes": "len_covered + bpp * sum(w h)", "peak_bytes_per_s": PEAK, "note": a.note, "cells": cells}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({cell: {k: v["median"] for k, v in c.items() if isinstance(v, dict)} for cell, c in cells.items()}))


if __name__ == "__main__":
    main()
