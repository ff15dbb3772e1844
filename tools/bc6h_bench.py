#!/usr/bin/env python3
"""BC6H granule-sorted field split (docs/BC6H_FORMAT.md) on one MI355X: forward and inverse time at 4 GiB, for a mode-mixed
buffer (every class, the reserved encodings included) and a single-mode buffer, each at an aligned block count (2^28) and at
2^28 + 1.  Every case checks the round trip and two sampled granules against tests/bc6h_ref.py.  Prints ONE JSON line with
the fraction of the 8 TB/s HBM peak on algorithmic bytes (2 * len).
    python tools/bc6h_bench.py [gib]          STEPS (default 10), WARM_MS (default 150)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bc6h_ref as R  # noqa: E402
import dxt_lossless_transform_amd as pkg  # noqa: E402
from dxt_lossless_transform_amd import bc6h  # noqa: E402

gib = float(sys.argv[1]) if len(sys.argv) > 1 else 4.0
steps = int(os.environ.get("STEPS", "10"))
warm_ms = float(os.environ.get("WARM_MS", "150"))
dev = torch.device("cuda:0")


def make(n: int, mix: str) -> torch.Tensor:
    x = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    pkg.fill_splitmix64(x, 0x0BC60001)
    b = x.view(-1, 16)
    codes = torch.tensor(list(R.MODE_BITS) + [19], dtype=torch.uint8, device=dev)
    k = (b[:, 15].to(torch.int64) % 15) if mix == "mixed" else torch.full((n,), 12, dtype=torch.int64, device=dev)
    mb = torch.where(k <= 1, 3, 0x1F).to(torch.uint8)
    b[:, 0] = (b[:, 0] & ~mb) | codes[k]
    return x


def check_granules(x: torch.Tensor, y: torch.Tensor, n: int) -> bool:
    main = n - n % 1024
    for g in (1, main // 1024 - 1):
        part = R.transform(x[16 * 1024 * g:16 * 1024 * (g + 1)].cpu().numpy())
        for o, w in zip(R.STREAM_OFF, R.STREAM_WIDTH):
            got = y[o * main + w * 1024 * g:o * main + w * 1024 * (g + 1)].cpu().numpy()
            if not np.array_equal(got, part[o * 1024:(o + w) * 1024]):
                return False
    return True


def run(n: int, mix: str) -> dict:
    x = make(n, mix)
    y, z = torch.empty_like(x), torch.empty_like(x)
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < warm_ms:   # steady clocks first (tools/bc7_bench.py has the reason)
        for _ in range(4):
            bc6h.transform_bc6h(x, y)
            bc6h.untransform_bc6h(y, z)
        torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    for k in range(steps):
        ev[k][0].record()
        bc6h.transform_bc6h(x, y)
        ev[k][1].record()
        bc6h.untransform_bc6h(y, z)
        ev[k][2].record()
    torch.cuda.synchronize()
    fwd = sum(e[0].elapsed_time(e[1]) for e in ev) / steps
    inv = sum(e[1].elapsed_time(e[2]) for e in ev) / steps
    nbytes = x.numel()
    out = {"blocks": n, "modes": mix, "roundtrip_exact": bool(torch.equal(z, x)), "granules_match_ref": check_granules(x, y, n),
           "fwd_ms": round(fwd, 3), "inv_ms": round(inv, 3),
           "fwd_frac_of_8TBps_on_2len": round(2 * nbytes / (fwd * 1e-3) / 8e12, 4),
           "inv_frac_of_8TBps_on_2len": round(2 * nbytes / (inv * 1e-3) / 8e12, 4)}
    del x, y, z
    torch.cuda.empty_cache()
    return out


aligned = int(gib * (1 << 30)) // 16
cases = [run(n, mix) for mix in ("mixed", "single") for n in (aligned, aligned + 1)]
print(json.dumps({"workload": f"BC6H granule-sorted field split v1, {gib:g} GiB", "steps": steps, "cases": cases}))
