"""Host time of dxtlt_transform_batch_device for one library (DXTLT_LIB_PATH): the mixed calls of tools/batch_mixed_host_probe.py
(16 calls of 96 items, BC1 fwd / BC7 fwd / BC7 inv), a call with 64 tile launches, the corpus call of bench.py (2130 BC1 items),
and the corpus legs' wall-clock value; medians and quartiles over many repetitions, one JSON line.  For an A/B run it once per
library in fresh processes that alternate (tools/ab_build_rev.sh builds the other one); profiles/batch_plan_refactor_host_time.txt.
usage: python tools/batch_call_host_time.py LABEL [groups]      (groups: the 64-launch call alone, five blocks of 200 calls)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import dxt_lossless_transform_amd as pkg
from dxt_lossless_transform_amd import batch
from oracle import oracle_c

pkg.load()
dev = torch.device("cuda:0")
out = {"label": sys.argv[1], "library": pkg._lib.lib_path()}


def enqueue_us(calls, reps):
    """median and quartiles over `reps` of the host time to enqueue `calls` back to back (the device idle at the start), in us"""
    for p in calls:
        batch.run_prepared_batch(p)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for p in calls:
            batch.run_prepared_batch(p)
        ts.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
    q = statistics.quantiles(ts, n=4)
    return {"median": round(statistics.median(ts), 1), "q1": round(q[0], 1), "q3": round(q[2], 1), "min": round(min(ts), 1)}


# many groups: 4 items of 64 KiB for each of BC1 (8 settings), BC2 (8), BC3 (16), forward and inverse: 64 launches per call
x = torch.from_numpy(oracle_c.fill_splitmix64(64 << 10, 5)).to(dev)
its = []
for fmt, cls, alphas in (("bc1", pkg.Bc1TransformSettings, (None,)), ("bc2", pkg.Bc2TransformSettings, (None,)),
                         ("bc3", pkg.Bc3TransformSettings, (False, True))):
    for mode in range(4):
        for sc in (False, True):
            for sa in alphas:
                s = cls(pkg.YCoCgVariant(mode), sc) if sa is None else cls(pkg.YCoCgVariant(mode), sa, sc)
                for inverse in (False, True):
                    for _ in range(4):
                        its.append((fmt, inverse, x, torch.empty_like(x), s))
groups = batch.prepare_batch(its)
if sys.argv[2:] == ["groups"]:
    # (the level of this call moves between processes and inside one, for any library: several blocks show it)
    out["block_medians_us"] = [enqueue_us([groups], 200)["median"] for _ in range(5)]
    out["median_us"] = statistics.median(out["block_medians_us"])
    print(json.dumps(out), flush=True)
    sys.exit(0)
out["groups_64x4_us"] = enqueue_us([groups], 200)

# the probe's mixed calls
n = 1 << 20
st = pkg.Bc1TransformSettings()
src7 = np.random.default_rng(7).integers(0, 256, n, dtype=np.uint8)
tr7 = oracle_c.transform_bc7(src7)
src1 = oracle_c.fill_splitmix64(n, 11)
calls = []
for c in range(16):
    its = []
    for i in range(96):
        kind = i % 3
        xd = torch.from_numpy((src1, src7, tr7)[kind]).to(dev)
        its.append((("bc1", "bc7", "bc7")[kind], kind == 2, xd, torch.empty_like(xd), st if kind == 0 else None))
    calls.append(batch.prepare_batch(its))
out["mixed_16x96_us"] = enqueue_us(calls, 200)
del calls

# the corpus call: enqueue time of one forward call of 2130 BC1 textures, then the legs as bench.py runs them
texs = bench.corpus_textures(1.0)
offs, arena = bench.corpus_layout(texs, 8, 256)
xa = torch.zeros(arena, dtype=torch.uint8, device=dev)
ya = torch.zeros(arena, dtype=torch.uint8, device=dev)
prep = batch.prepare_batch([("bc1", False, xa[o:o + b * 8], ya[o:o + b * 8], st) for (_, _, b), o in zip(texs, offs)])
out["corpus_bc1_call_us"] = enqueue_us([prep], 60)
out["corpus_items"] = len(texs)
del prep, xa, ya
torch.cuda.empty_cache()
for name, fmt in (("corpus", "bc1"), ("corpus_bc3", "bc3")):
    leg = bench.run_corpus_leg(pkg, torch, dev, fmt, 10, 2, 1.0, cpu=False)
    assert leg["bit_exact_roundtrip"] and leg["oracle_textures_exact"] and leg["forward_gaps_exact"], leg
    out[name] = {"wall_GiBps": leg["value"], "fwd_ms": leg["fwd_ms"], "inv_ms": leg["inv_ms"]}
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
