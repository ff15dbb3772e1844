#!/usr/bin/env python3
"""BC4 / BC5 transforms (docs/BC45_FORMAT.md) on 8 GiB synthetic buffers, one MI355X: forward and inverse for both formats and both
settings, at an aligned block count (8 GiB exactly: every stream on its 128-byte line, aligned tiles) and at 2^k + 1 blocks (every
stream base off its line: halo / shifted tiles plus edge tiles).  Checks the round trip and a sampled window of the transformed
buffer against the layout table, and prints ONE JSON line: GiB/s and the fraction of the 8 TB/s peak on algorithmic bytes (2 * len).
    python tools/bc45_bench.py [GiB=8] [STEPS env, default 20]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bc45_ref  # noqa: E402
import dxt_lossless_transform_amd as pkg  # noqa: E402

gib = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
steps = int(os.environ.get("STEPS", "20"))
warm_ms = float(os.environ.get("WARM_MS", "150"))   # steady clocks first (tools/bc7_bench.py, profiles/r03_clock_ramp.txt)
dev = torch.device("cuda:0")
max_bytes = int(gib * (1 << 30)) + 16
x_all = torch.empty(max_bytes, dtype=torch.uint8, device=dev)
y_all, z_all = torch.empty_like(x_all), torch.empty_like(x_all)
pkg.fill_splitmix64(x_all, 0x0BC45000)


def window_ok(fmt, split, x, y, n):
    """a window of blocks in the middle of the buffer, stream by stream, against the layout table"""
    B = bc45_ref.BLOCK[fmt]
    a, w = n // 2 - 1000, 4099
    aos = x[a * B:(a + w) * B].cpu().numpy().reshape(w, B)
    for off, width in bc45_ref.streams(fmt, split):
        got = y[off * n + width * a:off * n + width * (a + w)].cpu().numpy()
        if not np.array_equal(got, aos[:, off:off + width].reshape(-1)):
            return False
    return True


results = []
for fmt in ("bc4", "bc5"):
    B = bc45_ref.BLOCK[fmt]
    aligned = int(gib * (1 << 30)) // B
    k = aligned.bit_length() - 1
    for count_kind, n in (("aligned", aligned), ("2^k+1", (1 << k) + 1)):
        x, y, z = x_all[:n * B], y_all[:n * B], z_all[:n * B]
        for split in (False, True):
            st = (pkg.Bc4TransformSettings if fmt == "bc4" else pkg.Bc5TransformSettings)(split)
            fwd_fn = getattr(pkg, f"transform_{fmt}_with_settings")
            inv_fn = getattr(pkg, f"untransform_{fmt}_with_settings")
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < warm_ms:
                for _ in range(4):
                    fwd_fn(x, y, st)
                    inv_fn(y, z, st)
                torch.cuda.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
            for s in range(steps):
                ev[s][0].record()
                fwd_fn(x, y, st)
                ev[s][1].record()
                inv_fn(y, z, st)
                ev[s][2].record()
            torch.cuda.synchronize()
            fwd = sorted(e[0].elapsed_time(e[1]) for e in ev)[steps // 2]   # medians, ms
            inv = sorted(e[1].elapsed_time(e[2]) for e in ev)[steps // 2]
            nbytes = n * B
            results.append({
                "format": fmt, "split_endpoints": split, "blocks": n, "count": count_kind, "bytes": nbytes,
                "fwd_ms": round(fwd, 3), "inv_ms": round(inv, 3),
                "fwd_GiBps": round(nbytes / (fwd * 1e-3) / 2**30, 1), "inv_GiBps": round(nbytes / (inv * 1e-3) / 2**30, 1),
                "fwd_frac": round(2 * nbytes / (fwd * 1e-3) / 8e12, 4), "inv_frac": round(2 * nbytes / (inv * 1e-3) / 8e12, 4),
                "roundtrip_exact": bool(torch.equal(z, x)), "window_exact": window_ok(fmt, split, x, y, n),
            })
            print(json.dumps(results[-1]), file=sys.stderr, flush=True)

ok = all(r["roundtrip_exact"] and r["window_exact"] for r in results)
print(json.dumps({"workload": f"BC4 / BC5 transforms, {gib:g} GiB, median of {steps}", "peak_TBps": 8.0, "all_exact": ok,
                  "results": results}))
sys.exit(0 if ok else 1)
