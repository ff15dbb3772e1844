#!/usr/bin/env python3
"""dxtlt_transform_batch_auto_device against what a caller had before it: a loop of dxtlt_transform_bcN_auto_device over the same
device-resident items.  One process, one device; every figure is the median of `--reps` runs after `--warmup`, HIP events around
the whole call (or the whole loop) plus a final stream synchronise.

Shapes: the 2130 BC1 textures of bench.py's corpus leg (the reference's published benchmark: mip-chained textures, odd block
counts), 8000 x 5463 blocks (a 256 x 256 texture with its mip chain), 1024 x 1 MiB, each with the fast and the all-modes search,
and the 8000 x 5463 shape as BC3.  Items lie side by side at 256-byte boundaries.  Data: blocks drawn at random from the
reference's 256 x 256 test texture of the format with the low two bits of both colour endpoints jittered (texture-like endpoint
sections; the estimator's LDS atomics see real collisions).

Phases, each the median of `--reps` further runs: `candidates` and `estimator` are HIP events the call records itself around the
candidate launches and the estimator launch of every chunk (dxtlt_debug_batch_auto_time_phases), summed over the chunks;
`transform` is the winners alone (dxtlt_transform_batch_device with the chosen settings); `rest` = the untimed call minus the
three: counter clear, table upload, readback, the wait and the host's planning (a difference of medians of separate runs: it
can come out a few tenths of a millisecond below zero).  `distinct_choices` says into how many settings
the winners fall: with this data every item of a shape picks the same, so the transform phase is ONE batch launch -- a corpus
whose textures favour different settings has a few.

Writes profiles/batch_auto_bench.json.   usage: python tools/batch_auto_bench.py [--reps 5] [--warmup 2] [--scale 1.0]
[--shapes corpus,tiny,mib,tiny_bc3] [--out profiles/batch_auto_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import dxt_lossless_transform_amd as pkg  # noqa: E402
from dxt_lossless_transform_amd import batch, estimator  # noqa: E402
from helpers import payload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--scale", type=float, default=1.0, help="item counts times this (a quick look)")
ap.add_argument("--shapes", default="corpus,tiny,mib,tiny_bc3")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_auto_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = estimator._l()


def shape_blocks(name):
    """-> (fmt, [blocks per item])"""
    n = lambda c: max(1, int(round(c * args.scale)))      # noqa: E731
    if name == "corpus":
        return "bc1", [t[2] for t in bench.corpus_textures(args.scale)]
    if name == "tiny":
        return "bc1", [5463] * n(8000)
    if name == "mib":
        return "bc1", [(1 << 20) // 8] * n(1024)
    if name == "tiny_bc3":
        return "bc3", [5463] * n(8000)
    raise SystemExit(f"unknown shape {name}")


def texture_like(fmt, total_blocks):
    B = pkg.BLOCK_BYTES[fmt]
    tex = torch.from_numpy(payload(fmt).reshape(-1, B).copy()).to(dev)
    g = torch.Generator(device=dev).manual_seed(0xBA7C + B)
    x = tex[torch.randint(0, tex.shape[0], (total_blocks,), device=dev, generator=g)]
    colour = 0 if fmt == "bc1" else 8
    for c in (colour, colour + 2):
        x[:, c] ^= torch.randint(0, 4, (total_blocks,), device=dev, generator=g, dtype=torch.uint8)
    return x.reshape(-1)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.current_stream().synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "scale": args.scale,
          "method": "median over reps of HIP events around the whole call / the whole loop, plus a final stream synchronise; one process",
          "shapes": {}}
for name in args.shapes.split(","):
    fmt, blocks = shape_blocks(name)
    B = pkg.BLOCK_BYTES[fmt]
    offs, at = [], 0
    for nb in blocks:
        offs.append(at)
        at = (at + nb * B + 255) // 256 * 256
    src = torch.zeros(at, dtype=torch.uint8, device=dev)
    data = texture_like(fmt, sum(blocks))
    pos = 0
    for o, nb in zip(offs, blocks):
        src[o:o + nb * B] = data[pos:pos + nb * B]
        pos += nb * B
    del data
    dst = torch.zeros_like(src)
    payload_bytes = sum(blocks) * B
    for use_all in (False, True) if fmt == "bc1" else (False,):
        arr = (estimator.BatchAutoItem * len(blocks))()
        for a, o, nb in zip(arr, offs, blocks):
            a.d_input, a.d_output, a.len = src.data_ptr() + o, dst.data_ptr() + o, nb * B
            a.format, a.use_all_decorrelation_modes = pkg._FMT_ID[fmt], int(use_all)
        stream = torch.cuda.current_stream().cuda_stream

        def batched():
            rc = lib.dxtlt_transform_batch_auto_device(arr, len(arr), stream)
            assert rc == 0, pkg._lib.last_error()

        single = getattr(lib, f"dxtlt_transform_{fmt}_auto_device")
        m, sa, sc = C.c_uint8(), C.c_bool(), C.c_bool()
        outs = (C.byref(m), C.byref(sc)) if fmt == "bc1" else (C.byref(m), C.byref(sa), C.byref(sc))

        def loop():
            for a in arr:
                rc = single(a.d_input, a.d_output, a.len, use_all, stream, *outs)
                assert rc == 0, pkg._lib.last_error()

        batch_ms, batch_all = timed(batched)
        stats = estimator.last_batch_auto()
        want = dst.clone()
        choices = [(a.decorrelation_mode, a.split_alpha_endpoints, a.split_colour_endpoints) for a in arr]
        loop_ms, loop_all = timed(loop)
        torch.cuda.synchronize()
        assert torch.equal(dst, want), "the loop and the batched call must leave the same bytes"
        # the winners alone
        win = (batch.DxtltBatchItem * len(arr))()
        for w, a in zip(win, arr):
            w.d_input, w.d_output, w.len, w.format = a.d_input, a.d_output, a.len, a.format
            w.decorrelation_mode, w.split_alpha_endpoints, w.split_colour_endpoints = a.decorrelation_mode, a.split_alpha_endpoints, a.split_colour_endpoints
        transform_ms, _ = timed(lambda: batch.run_prepared_batch((win, dev, None)))
        phase_runs = []

        def phased():
            batched()
            out = (C.c_double * 2)()
            lib.dxtlt_debug_batch_auto_last_phase_ms(out)
            phase_runs.append((out[0], out[1]))

        lib.dxtlt_debug_batch_auto_time_phases(1)
        try:
            timed(phased)
        finally:
            lib.dxtlt_debug_batch_auto_time_phases(0)
        candidates_ms = statistics.median(r[0] for r in phase_runs[args.warmup:])
        estimator_ms = statistics.median(r[1] for r in phase_runs[args.warmup:])
        key = f"{name}_{'all' if use_all else 'fast'}"
        result["shapes"][key] = {
            "format": fmt, "items": len(blocks), "payload_MiB": round(payload_bytes / 2**20, 1), "use_all": use_all,
            "batched_ms": round(batch_ms, 3), "loop_ms": round(loop_ms, 3), "loop_over_batched": round(loop_ms / batch_ms, 2),
            "batched_GiB_per_s": round(payload_bytes / 2**30 / (batch_ms / 1e3), 1), "loop_GiB_per_s": round(payload_bytes / 2**30 / (loop_ms / 1e3), 1),
            "phases_ms": {"candidates": round(candidates_ms, 3), "estimator": round(estimator_ms, 3), "transform": round(transform_ms, 3),
                          "rest": round(batch_ms - candidates_ms - estimator_ms - transform_ms, 3)},
            "stream_waits, chunks, candidate launches, estimator launches": list(stats),
            "distinct_choices": len(set(choices)), "batched_ms_all": [round(v, 3) for v in batch_all], "loop_ms_all": [round(v, 3) for v in loop_all],
            "not_slower_than_the_loop": batch_ms <= loop_ms,
        }
        print(key, json.dumps(result["shapes"][key]), flush=True)
    del src, dst
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
