#!/usr/bin/env python3
"""Per-call time of the single-buffer auto calls, two builds of the library side by side on one GPU: the figure that moves when
the HOST code on the call path changes (the kernels bound the large sizes).  Every library runs in a fresh process of its own,
the old and the new one alternating (old, new, old, new); the old library's two runs give its own run-to-run spread per cell.

    tools/ab_build.sh HEAD~1 auto_transform.cpp        # or a whole parent build copied to ab/libdxtlt_old.so
    python tools/auto_call_ab.py --old ab/libdxtlt_old.so --new dxt-lossless-transform_amd/libdxtlt_gfx950.so --out result.json

A cell is (call, size): warmed up, then timed in windows of at least half a second each (call + wait for the stream); the
figure of a run is the median over its windows of the window's time per call.  A cell passes when the new library's median is
at most the old one's plus the larger of the old one's spread and 2 %."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64 << 10, 16 << 20, 1 << 30)
CALLS = ("bc1_auto_device", "bc3_auto_device", "bc1_auto_with_normalization_device", "pixels_auto_device", "bc1_auto_host_builtin",
         "bc1_auto_with_normalization_host_builtin")


def tiled(chunk, nbytes):
    import numpy as np

    return np.ascontiguousarray(np.tile(chunk, nbytes // chunk.size))


def run_cells(lib_path):
    """every cell with the library at lib_path; prints one JSON object {call: {size: seconds per call}}"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import auto_normalize_ref as A

    lib = C.CDLL(lib_path)
    vp, sz, b, i32 = C.c_void_p, C.c_size_t, C.c_bool, C.c_int32
    lib.dxtlt_builtin_size_estimator.restype = vp
    lib.dxtlt_last_error.restype = C.c_char_p
    for name, args in (("dxtlt_transform_bc1_auto_device", [vp, vp, sz, b, vp, vp, vp]),
                       ("dxtlt_transform_bc3_auto_device", [vp, vp, sz, b, vp, vp, vp, vp]),
                       ("dxtlt_transform_bc1_auto_with_normalization_device", [vp, vp, sz, b, vp, vp, vp, vp]),
                       ("dxtlt_transform_pixels_auto_device", [vp, vp, sz, i32, vp, vp, vp]),
                       ("dxtlt_transform_bc1_auto", [vp, vp, sz, vp, b, vp, vp, vp]),
                       ("dxtlt_transform_bc1_auto_with_normalization", [vp, vp, sz, vp, b, vp, vp, vp, vp])):
        f = getattr(lib, name)
        f.argtypes, f.restype = args, i32
    builtin = lib.dxtlt_builtin_size_estimator()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0xAB)
    noise = rng.integers(0, 256, 64 << 10, dtype=np.uint8)
    normalisable = A.blocks(1, "cycle", 8192)               # 64 KiB of BC1 blocks, every class of block in every slot
    out = {}
    for call in CALLS:
        out[call] = {}
        for nbytes in SIZES:
            x = tiled(normalisable if "normalization" in call else noise, nbytes)
            if call.endswith("_device"):
                d_x = torch.from_numpy(x).to(dev)
                d_y = torch.empty_like(d_x)
                src, dst = d_x.data_ptr(), d_y.data_ptr()
            else:
                y = np.empty_like(x)
                src, dst = x.ctypes.data, y.ctypes.data
            one = {"bc1_auto_device": lambda: lib.dxtlt_transform_bc1_auto_device(src, dst, nbytes, False, stream, None, None),
                   "bc3_auto_device": lambda: lib.dxtlt_transform_bc3_auto_device(src, dst, nbytes, False, stream, None, None, None),
                   "bc1_auto_with_normalization_device":
                       lambda: lib.dxtlt_transform_bc1_auto_with_normalization_device(src, dst, nbytes, False, stream, None, None, None),
                   "pixels_auto_device": lambda: lib.dxtlt_transform_pixels_auto_device(src, dst, nbytes, 4, stream, None, None),
                   "bc1_auto_host_builtin": lambda: lib.dxtlt_transform_bc1_auto(src, dst, nbytes, builtin, False, None, None, None),
                   "bc1_auto_with_normalization_host_builtin":
                       lambda: lib.dxtlt_transform_bc1_auto_with_normalization(src, dst, nbytes, builtin, False, None, None, None, None)}[call]

            def timed(calls):
                t = time.perf_counter()
                for _ in range(calls):
                    rc = one()
                    torch.cuda.synchronize()
                    assert rc == 0, (call, nbytes, rc, lib.dxtlt_last_error())
                return time.perf_counter() - t

            timed(3)                                          # warm-up: the arena, the staging buffers, the code objects
            calls = max(1, int(0.55 / (timed(3) / 3)) + 1)    # a window of at least half a second
            windows = []
            while len(windows) < (5 if nbytes < (1 << 30) else 3):
                dt = timed(calls)
                if dt < 0.5:                                  # the calls got faster: a longer window, this one does not count
                    calls = int(calls * 0.6 / dt) + 1
                    continue
                windows.append(dt / calls)
            out[call][str(nbytes)] = statistics.median(windows)
            del x
            if call.endswith("_device"):
                del d_x, d_y
                torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old")
    ap.add_argument("--new")
    ap.add_argument("--out")
    ap.add_argument("--cells", help="(internal) run every cell with this library")
    a = ap.parse_args()
    if a.cells:
        return run_cells(a.cells)
    runs = []
    for which in ("old", "new", "old", "new"):
        path = os.path.abspath(a.old if which == "old" else a.new)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cells", path], capture_output=True, text=True, timeout=420)
        if p.returncode != 0:                                 # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            return p.returncode
        runs.append((which, json.loads(next(line for line in p.stdout.splitlines() if line.startswith("RESULT "))[7:])))
        print(which, "done", flush=True)
    cells, ok = [], True
    for call in CALLS:
        for nbytes in SIZES:
            old = [r[call][str(nbytes)] for w, r in runs if w == "old"]
            new = [r[call][str(nbytes)] for w, r in runs if w == "new"]
            old_median, new_median = statistics.median(old), statistics.median(new)
            spread = (max(old) - min(old)) / old_median
            margin = max(spread, 0.02)
            passed = new_median <= old_median * (1 + margin)
            ok = ok and passed
            cells.append({"call": call, "bytes": nbytes, "old_us": [round(t * 1e6, 2) for t in old], "new_us": [round(t * 1e6, 2) for t in new],
                          "old_median_us": round(old_median * 1e6, 2), "new_median_us": round(new_median * 1e6, 2),
                          "old_spread": round(spread, 4), "margin": round(margin, 4), "new_over_old": round(new_median / old_median, 4),
                          "pass": passed})
            print(f"{call:42s} {nbytes:>11d}  old {old_median * 1e6:12.2f} us  new {new_median * 1e6:12.2f} us  "
                  f"new/old {new_median / old_median:.4f}  spread {spread:.4f}  {'pass' if passed else 'OUTSIDE'}", flush=True)
    result = {"command": "python tools/auto_call_ab.py --old " + a.old + " --new " + a.new, "order": [w for w, _r in runs],
              "rule": "new median <= old median * (1 + max(old spread, 0.02)); a run's figure: median of its >= 0.5 s windows",
              "all_pass": ok, "cells": cells}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
