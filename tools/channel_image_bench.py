#!/usr/bin/env python3
"""Fused BC4 / BC5 untransform + image decode (include/dxtlt_image.h, the *_channel_image calls) against the two calls it replaces.

Per format (BC4, BC5; split_endpoints = false, the settings types' default) and per block count (the image's own: aligned tiles; one
extra block in the transformed buffer, so that total_blocks is odd: shifted tiles), HIP-event times after a warm-up of
  (a) dxtlt_untransform_decode_channel_image_device                                 -- must move len + bpp w h bytes
  (b) dxtlt_untransform_bc{4,5}_with_settings_device into a scratch buffer, then
      dxtlt_decode_channel_image_device from it                                      -- must move 2 len, then len + bpp w h
      (timed together and each part on its own)
  (c) the BC3 fused call dxtlt_untransform_decode_image_device on an image of the same size, default settings, in the same
      process: what a fused image kernel reaches on this box today
and the fraction of the 8 TB/s HBM peak each reaches on those bytes.  Before a cell is timed, three rows of (a)'s image are compared
with the CPU statement (tests/channel_image_ref.py).  Every cell is measured in `--processes` fresh processes, one after the
other, each under a time limit of its own; the first one that fails ends the run.  The file keeps every sample, the median and
the spread.

--ab-lib PATH [--ab-label NAME]: (a) once more per process with another build of the library (DXTLT_LIB_PATH), for an A/B of
two forms of the kernel; recorded under "ab".

    python tools/channel_image_bench.py [--size 16384] [--steps 1000] [--processes 3] [--out profiles/channel_image_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK = 8e12
FMT_ID = {"bc4": 4, "bc5": 5}
BLOCK = {"bc4": 8, "bc5": 16}
BPP = {"bc4": 1, "bc5": 2}
SPLIT = False


def child(size, steps, fused_only):
    """one process: every cell once; prints one JSON line"""
    import time

    import numpy as np
    import torch

    import channel_image_ref
    import dxt_lossless_transform_amd as pkg
    from dxt_lossless_transform_amd import image
    from oracle import oracle_c

    dev = torch.device("cuda:0")
    img = image._l()
    lib = pkg.load()
    w = h = size
    bpr = (w + 3) // 4
    blocks = image.image_blocks(w, h)
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

    def best_of_two(*fns):
        """the variants alternated, twice each; the better time of each"""
        ms = [float("inf")] * len(fns)
        for _ in range(2):
            for i, fn in enumerate(fns):
                ms[i] = min(ms[i], timed(fn))
        return ms

    out = {}
    for fmt in ("bc4", "bc5"):
        bs, bpp = BLOCK[fmt], BPP[fmt]
        pitch = bpp * w
        pixels = torch.empty(pitch * h, dtype=torch.uint8, device=dev)
        settings = {"bc4": pkg.Bc4TransformSettings(SPLIT), "bc5": pkg.Bc5TransformSettings(SPLIT)}[fmt]
        forward = getattr(pkg, f"transform_{fmt}_with_settings")
        untransform = getattr(lib, f"dxtlt_untransform_{fmt}_with_settings_device")
        for label, total in (("aligned", blocks), ("odd_total", blocks + 1)):
            seed = 0xC4A70000 + 16 * FMT_ID[fmt] + (total & 1)
            length = total * bs
            x = torch.empty(length, dtype=torch.uint8, device=dev)
            t = torch.empty_like(x)
            pkg.fill_splitmix64(x, seed)
            forward(x, t, settings)
            torch.cuda.synchronize()

            def fused():
                rc = img.dxtlt_untransform_decode_channel_image_device(FMT_ID[fmt], t.data_ptr(), total, 0, w, h, SPLIT,
                                                                       pixels.data_ptr(), pitch, stream)
                assert rc == 0

            def untransform_only():
                rc = untransform(t.data_ptr(), x.data_ptr(), length, SPLIT, stream)
                assert rc == 0

            def decode_only():
                rc = img.dxtlt_decode_channel_image_device(FMT_ID[fmt], x.data_ptr(), w, h, pixels.data_ptr(), pitch, stream)
                assert rc == 0

            def two_calls():
                untransform_only()
                decode_only()

            # exactness first: three rows of the fused call's image (and of the plain decoder's) against the CPU statement
            for run in (fused,) if fused_only else (fused, two_calls):
                pixels.zero_()
                run()
                torch.cuda.synchronize()
                for y in (1, h // 2 + 2, h - 1):
                    by = y // 4
                    row_blocks = oracle_c.fill_splitmix64(bpr * bs, seed, by * bpr * bs // 8)
                    want = channel_image_ref.decode_blocks(oracle_c, fmt, row_blocks).reshape(bpr, 4, 4, bpp)[:, y % 4].reshape(-1)
                    got = pixels[y * pitch:y * pitch + bpp * w].cpu().numpy()
                    assert np.array_equal(got, want[:bpp * w]), (fmt, label, y, run.__name__)
            bytes_a = length + bpp * w * h
            if fused_only:
                ms_a, = best_of_two(fused)
                out[f"{fmt}_{label}"] = {"fused_ms": round(ms_a, 4), "fused_peak": round(bytes_a / (ms_a * 1e-3) / PEAK, 4)}
            else:
                ms_a, ms_b, ms_u, ms_d = best_of_two(fused, two_calls, untransform_only, decode_only)
                out[f"{fmt}_{label}"] = {
                    "fused_ms": round(ms_a, 4), "fused_peak": round(bytes_a / (ms_a * 1e-3) / PEAK, 4),
                    "two_calls_ms": round(ms_b, 4), "two_calls_peak": round((2 * length + bytes_a) / (ms_b * 1e-3) / PEAK, 4),
                    "untransform_ms": round(ms_u, 4), "untransform_peak": round(2 * length / (ms_u * 1e-3) / PEAK, 4),
                    "decode_ms": round(ms_d, 4), "decode_peak": round(bytes_a / (ms_d * 1e-3) / PEAK, 4)}
            del x, t
        del pixels
    if not fused_only:
        # (c) the yardstick: BC3, default settings, the same image size, RGBA8888
        pitch = 4 * w
        pixels = torch.empty(pitch * h, dtype=torch.uint8, device=dev)
        for label, total in (("aligned", blocks), ("odd_total", blocks + 1)):
            length = total * 16
            x = torch.empty(length, dtype=torch.uint8, device=dev)
            t = torch.empty_like(x)
            pkg.fill_splitmix64(x, 0xC4A70030 + (total & 1))
            pkg.transform_bc3_with_settings(x, t, pkg.Bc3TransformSettings())
            torch.cuda.synchronize()

            def bc3_fused():
                rc = img.dxtlt_untransform_decode_image_device(3, t.data_ptr(), total, 0, w, h, 1, True, True, pixels.data_ptr(), pitch,
                                                               stream)
                assert rc == 0

            ms_c, = best_of_two(bc3_fused)
            out[f"bc3_{label}"] = {"fused_ms": round(ms_c, 4), "fused_peak": round((length + 4 * w * h) / (ms_c * 1e-3) / PEAK, 4)}
            del x, t
    print("RESULT " + json.dumps(out))


def run_children(a, fused_only, env=None):
    """`a.processes` fresh processes, one after the other, each under its own time limit; a failure ends the run (check=True)"""
    runs = []
    for _ in range(a.processes):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size),
               "--steps", str(a.steps)] + (["--fused-only"] if fused_only else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, env=env)
        runs.append(json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:]))
        print(f"process {len(runs)} of {a.processes} done", flush=True)
    return runs


def summarise(runs):
    cells = {}
    for cell in runs[0]:
        c = {}
        for key in runs[0][cell]:
            samples = [r[cell][key] for r in runs]
            c[key] = {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}
        cells[cell] = c
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_image_bench.json"))
    ap.add_argument("--ab-lib", default=None, help="another build of the library: the fused call once more per process with it")
    ap.add_argument("--ab-label", default="other build")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.size, a.steps, a.fused_only)
        return
    runs = run_children(a, False)   # this process never opens the device
    cells = summarise(runs)
    for cell, c in cells.items():
        if "two_calls_ms" not in c:
            continue
        c["fused_is_faster_in_every_process"] = all(r[cell]["fused_ms"] < r[cell]["two_calls_ms"] for r in runs)
        # the margin against the spread the processes show: the slowest fused sample against the fastest two-call sample
        c["slowest_fused_below_fastest_two_calls"] = c["fused_ms"]["max"] < c["two_calls_ms"]["min"]
        c["speedup_median"] = round(c["two_calls_ms"]["median"] / c["fused_ms"]["median"], 3)
        c["fused_peak_minus_bc3_fused_peak"] = round(c["fused_peak"]["median"] - cells["bc3_" + cell.split("_", 1)[1]]["fused_peak"]["median"], 4)
    result = {"workload": f"{a.size} x {a.size} R8 / RG8 (BC3 yardstick: RGBA8888), split_endpoints false, {a.steps} steps per timing, "
                          f"{a.processes} processes",
              "bytes": {"fused": "len + bpp w h", "two_calls": "2 len + len + bpp w h", "untransform": "2 len", "decode": "len + bpp w h",
                        "bc3 fused": "len + 4 w h"},
              "peak_bytes_per_s": PEAK, "cells": cells}
    if a.ab_lib:
        env = dict(os.environ, DXTLT_LIB_PATH=os.path.abspath(a.ab_lib))
        ab = summarise(run_children(a, True, env))
        result["ab"] = {"label": a.ab_label, "cells": ab,
                        "this_build_over_other_ms": {cell: round(cells[cell]["fused_ms"]["median"] / ab[cell]["fused_ms"]["median"], 3)
                                                     for cell in ab}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({cell: {k: v["median"] for k, v in c.items() if isinstance(v, dict)} for cell, c in cells.items()}))
    if a.ab_lib:
        print(json.dumps({"ab " + a.ab_label: {cell: c["fused_ms"]["median"] for cell, c in result["ab"]["cells"].items()}}))


if __name__ == "__main__":
    main()
