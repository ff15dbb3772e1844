#!/usr/bin/env python3
"""BC1 forward transform with block normalisation fused in (reference experimental module) next to the plain forward
transform and the stand-alone normalise kernel: ms and fraction of the 8 TB/s HBM peak on the algorithmic 2*len.

    tools/normalize_bench.py [GIB] [mixed|random]                     the BC1 legs, one JSON line

    tools/normalize_bench.py bc23 [--gib 4] [--processes 3] [--out profiles/normalize_fused_bc23_bench.json]
        the BC2 / BC3 legs (dxtlt_transform_bc{2,3}_with_normalize_blocks_device).  Cells: format x block count (GIB aligned, and
        the same + 1 block) x settings (the format's default, all off) x modes (BC3 (1, 1) and (3, 2), BC2 colour modes 1 and 2).
        Every cell is timed in `processes` fresh processes; each times three things in the same process, alternating them in rounds:
          fused            the fused device call
          two_pass         the route without it: dxtlt_bcN_normalize_blocks_device into a scratch buffer, then dxtlt_transform_bcN_device
          plain            the plain dxtlt_transform_bcN_device
        ms per call (median of the rounds) and the fraction of the 8 TB/s HBM peak on the algorithmic 2 * len of ONE pass (two_pass
        moves 4 * len: its figure is the rate a caller sees for the operation).  Acceptance: fused is faster than two_pass in every
        cell and every process by more than the cell's run-to-run spread (largest max - min of a leg's ms over the processes).
    tools/normalize_bench.py bc23-cells --gib G                       one such process: a JSON line with every cell"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dxt_lossless_transform_amd as pkg  # noqa: E402
from dxt_lossless_transform_amd import normalize as norm  # noqa: E402



def event_ms(fn, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def bc23_cells(gib, rounds=5, steps=10):
    import statistics
    import time

    from dxt_lossless_transform_amd import normalize23 as n23

    dev = torch.device("cuda:0")
    out = {}
    for fmt in ("bc2", "bc3"):
        default = (1, True, True)
        transform = getattr(pkg, f"transform_{fmt}_with_settings")
        for extra in (0, 1):
            n = int(gib * (1 << 30)) // 16 + extra
            x = torch.empty(n * 16, dtype=torch.uint8, device=dev)
            pkg.fill_splitmix64(x, 0x0BC23E01)
            b = x.view(-1, 16)
            for lo in range(0, n, 1 << 25):   # 1/4 solid colour, 1/4 uniform opaque alpha (equal endpoints: the index walk), 1/4 both
                hi = min(n, lo + (1 << 25))
                k = torch.arange(lo, hi, device=dev) % 4
                v = b[lo:hi]
                v[(k & 1) == 1, 12:] = 0
                if fmt == "bc3":
                    v[k >= 2, 0:2] = 0xFF
                del k
            y, scratch = torch.empty_like(x), torch.empty_like(x)
            for s in (default, (0, False, False)):
                st = (pkg.Bc2TransformSettings(pkg.YCoCgVariant(s[0]), s[2]) if fmt == "bc2"
                      else pkg.Bc3TransformSettings(pkg.YCoCgVariant(s[0]), s[1], s[2]))
                for a, c in (((0, 1), (0, 2)) if fmt == "bc2" else ((1, 1), (3, 2))):
                    if fmt == "bc2":
                        fused = lambda: norm.transform_bc2_with_normalize_blocks(x, y, c, s[0], s[2])  # noqa: E731
                    else:
                        fused = lambda: norm.transform_bc3_with_normalize_blocks(x, y, a, c, s[0], s[1], s[2])  # noqa: E731

                    def two_pass():
                        n23.normalize_blocks(fmt, x, scratch, n23.ColorNormalizationMode(c), n23.AlphaNormalizationMode(a))
                        transform(scratch, y, st)

                    legs = {"fused": fused, "two_pass": two_pass, "plain": lambda: transform(x, y, st)}
                    t0 = time.perf_counter()
                    while time.perf_counter() - t0 < 0.1:   # warm up by wall time (clock ramp), every leg
                        for fn in legs.values():
                            fn()
                        torch.cuda.synchronize()
                    ms = {k: [] for k in legs}
                    for _ in range(rounds):
                        for k, fn in legs.items():
                            ms[k].append(event_ms(fn, steps))
                    cell = f"{fmt} blocks={n} settings=v{s[0]}-sa{int(s[1])}-sc{int(s[2])} modes=({a}, {c})"
                    out[cell] = {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                     "of_peak_on_2len": round(2 * x.numel() / (statistics.median(v) * 1e-3) / 8e12, 4)}
                                 for k, v in ms.items()}
            del x, y, scratch, b
            torch.cuda.empty_cache()
    return out


def bc23_main(argv):
    import argparse
    import subprocess

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "normalize_fused_bc23_bench.json"))
    a = ap.parse_args(argv)
    runs = []
    for _ in range(a.processes):   # one after the other: fresh processes, never two on the device at once
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "bc23-cells", "--gib", str(a.gib)], capture_output=True,
                              text=True, check=True)
        runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
    cells, accepted = {}, True
    for cell in runs[0]:
        legs = {k: [r[cell][k] for r in runs] for k in ("fused", "two_pass", "plain")}
        spread = max(max(p["ms"] for p in v) - min(p["ms"] for p in v) for v in legs.values())
        margins = [round(t["ms"] - f["ms"], 4) for f, t in zip(legs["fused"], legs["two_pass"])]
        ok = all(m > spread for m in margins)
        accepted = accepted and ok
        cells[cell] = {"processes": legs, "spread_ms": round(spread, 4), "two_pass_minus_fused_ms": margins,
                       "fused_over_plain": [round(f["ms"] / p["ms"], 4) for f, p in zip(legs["fused"], legs["plain"])],
                       "fused_faster_than_two_pass_by_more_than_the_spread": ok}
    res = {"workload": f"BC2 / BC3 forward transform with fused block normalisation, {a.gib:g} GiB per buffer, mixed blocks "
                       "(1/4 solid colour, 1/4 uniform opaque alpha, 1/4 both), device pointers",
           "legs": "ms per call, median / min / max of 5 rounds of 10 calls, the three legs alternating; of_peak_on_2len: 2 * len / ms / 8 TB/s",
           "processes_per_cell": a.processes, "accepted": accepted, "cells": cells}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"accepted": accepted, "out": a.out, "cells": len(cells)}))


if len(sys.argv) > 1 and sys.argv[1] == "bc23-cells":
    print(json.dumps(bc23_cells(float(sys.argv[sys.argv.index("--gib") + 1]) if "--gib" in sys.argv else 4.0)))
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "bc23":
    bc23_main(sys.argv[2:])
    sys.exit(0)

gib = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
share = sys.argv[2] if len(sys.argv) > 2 else "mixed"   # "mixed": 1/4 solid + 1/4 transparent blocks; "random": none
dev = torch.device("cuda:0")
n = int(gib * (1 << 30)) // 8
x = torch.empty(n * 8, dtype=torch.uint8, device=dev)
pkg.fill_splitmix64(x, 0x0BC14E01)
if share == "mixed":
    b = x.view(-1, 8)
    for lo in range(0, n, 1 << 26):   # in slices: boolean index temporaries are large
        hi = min(n, lo + (1 << 26))
        k = torch.arange(lo, hi, device=dev) % 4
        v = b[lo:hi]
        v[k == 1, 4:] = 0
        rows = (k == 2).nonzero().squeeze(1)
        v[rows, 0:2] = 0
        v[rows, 4:] = 0xFF
        del k, rows
y = torch.empty_like(x)
D = norm.Bc1TransformDetailsWithNormalization
M = norm.ColorNormalizationMode


def timed(fn, steps=10):
    import time as _t
    _t0 = _t.perf_counter()
    while (_t.perf_counter() - _t0) < 0.1:   # warm up by wall time: the chip ramps its clocks for ~40 ms after idling (profiles/r03_clock_ramp.txt)
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / steps
    return round(ms, 4), round(2 * x.numel() / (ms * 1e-3) / 8e12, 4)


res = {"workload": f"BC1 {gib:g} GiB, {share} blocks"}
res["plain_transform"] = timed(lambda: pkg.transform_bc1_with_settings(x, y))
for m in (M.COLOR0_ONLY, M.REPLICATE_COLOR):
    res[f"fused_{m.name.lower()}"] = timed(lambda: norm.transform_bc1_with_normalize_blocks(x, y, D(m, 1, True)))
res["normalize_only_color0"] = timed(lambda: norm.normalize_blocks(x, y, M.COLOR0_ONLY))
res["normalize_in_place"] = timed(lambda: norm.normalize_blocks(y, y, M.COLOR0_ONLY))
print(json.dumps(res))
