#!/usr/bin/env python3
"""Measures the built-in size estimator and the auto transforms that use it (include/dxtlt_estimator.h) on one GPU and writes
profiles/estimator_bench.json:

  * the kernel alone: 4 GiB of section bytes (16 sections in one launch), random and texture-like, after a 100 ms warm-up, for
    256 / 512 / 1024 lanes per workgroup and the (W, BITS) pairs (32768, 14) -- the estimator -- (32768, 13), (16384, 13) and
    (8192, 12), which fit two to six workgroups per CU; as bytes read per second and as a fraction of the 8 TB/s peak;
  * dxtlt_transform_bc{1,3}_auto_device on 1 GiB next to its parts, each timed alone in the same run with the same clock
    (events): the candidate kernel, the estimate launch over the arena's sections, one plain transform; gap = whole - sum;
  * host-pointer dxtlt_transform_bc1_auto on 256 MiB: the built-in vtable (device route) against a copy of it with wrapped
    function pointers (callback route, the same estimator); the two outputs and choices must be equal.

    python tools/estimator_bench.py [--out profiles/estimator_bench.json] [--small]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dxt_lossless_transform_amd as pkg  # noqa: E402
from dxt_lossless_transform_amd import estimator as E  # noqa: E402

PEAK = 8.0e12


def timed(fn, min_seconds=0.5, warm_seconds=0.1):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_seconds:
        fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 0, 0.0
    while total < min_seconds:
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b) / 1e3
        n += 1
    return total / n


def wall(fn, repeats=3):
    """mean host wall time of a synchronous call"""
    fn()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    return (time.perf_counter() - t0) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimator_bench.json"))
    ap.add_argument("--small", action="store_true", help="1/16 of every size (a quick look, not the record)")
    args = ap.parse_args()
    scale = 16 if args.small else 1
    dev = torch.device("cuda:0")
    pkg.build()
    l = E._l()
    res = {"device": torch.cuda.get_device_name(0), "estimator_version": E.version(), "peak_bytes_per_s": PEAK, "kernel": [], "auto_device": [],
           "auto_host": []}

    # ---- the kernel alone ----
    total = (4 << 30) // scale
    golden = np.fromfile(os.path.join(ROOT, "tests", "golden", "r2-256-bc1.payload.bin"), dtype=np.uint8)
    for kind in ("random", "texture"):
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        if kind == "random":
            pkg.fill_splitmix64(buf, 1)
        else:
            buf.view(-1, golden.size)[:] = torch.from_numpy(golden).to(dev)
            buf[:: 97] = 0x5A
        secs = list(buf.chunk(16))
        out = torch.zeros(16, dtype=torch.int64, device=dev)
        for w, bits in ((32768, 14), (32768, 13), (16384, 13), (8192, 12)):
            for lanes in (256, 512, 1024):
                dt = timed(lambda: E.estimate_sizes(secs, out, shape=(lanes, w, bits)))
                res["kernel"].append({"data": kind, "window": w, "bits": bits, "lanes": lanes, "lds_bytes": w + 32 + (4 << bits) + 4,
                                      "bytes": total, "seconds": dt, "bytes_per_s": total / dt, "fraction_of_peak": total / dt / PEAK,
                                      "estimate_over_len": float(out.sum().item()) / total})
                print(res["kernel"][-1], flush=True)
        del buf, secs

    # ---- auto on device pointers ----
    n = (1 << 30) // scale
    x = torch.empty(n, dtype=torch.uint8, device=dev)
    pkg.fill_splitmix64(x, 2)
    y = torch.empty_like(x)
    for fmt in ("bc1", "bc3"):
        code = 1 if fmt == "bc1" else 3
        for use_all in (False, True):
            stream = torch.cuda.current_stream().cuda_stream
            t_auto = timed(lambda: E.transform_auto(fmt, x, y, use_all))
            t_plain = timed(lambda: getattr(pkg, f"transform_{fmt}_with_settings")(x, y))

            def candidates():
                rc = l.dxtlt_debug_auto_candidates_device(code, use_all, x.data_ptr(), n, stream)
                assert rc == 0, rc
            t_cand = timed(candidates)
            # the estimate launch over sections of the arena's sizes (their bytes: the input's, which is as random as the arena's)
            colour = n // 2 if fmt == "bc1" else n // 4
            sections = [x[k * colour % (n - colour):][:colour] for k in range(8 if use_all else 4)] + ([x[:n // 8], x[n // 8:n // 4]] if fmt == "bc3" else [])
            out = torch.zeros(len(sections), dtype=torch.int64, device=dev)
            t_est = timed(lambda: E.estimate_sizes(sections, out))
            parts = t_cand + t_est + t_plain
            res["auto_device"].append({"format": fmt, "use_all": use_all, "bytes": n, "auto_seconds": t_auto, "candidate_kernel_seconds": t_cand,
                                       "estimate_launch_seconds": t_est, "plain_transform_seconds": t_plain, "sum_of_parts_seconds": parts,
                                       "gap_over_sum": (t_auto - parts) / parts, "bytes_per_s": n / t_auto})
            print(res["auto_device"][-1], flush=True)
    del x, y

    # ---- auto on host pointers: device route against callback route, the same estimator ----
    n = (256 << 20) // scale
    hx = np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8)
    hy = np.zeros_like(hx)
    builtin = E.builtin_size_estimator()
    inner_max, inner_est = builtin.contents.MaxCompressedSize, builtin.contents.EstimateCompressedSize
    wrapped_max = E.MAXFN(lambda ctx, ln, o: inner_max(ctx, ln, o))
    wrapped_est = E.ESTFN(lambda ctx, p, ln, s, sl, o: inner_est(ctx, p, ln, s, sl, o))
    wrapped = E.DltSizeEstimator(None, wrapped_max, wrapped_est)
    m, c = C.c_uint8(), C.c_bool()
    outputs = []
    for name, est in (("builtin", builtin), ("wrapped_callbacks", C.pointer(wrapped))):
        def call():
            rc = l.dxtlt_transform_bc1_auto(hx.ctypes.data, hy.ctypes.data, n, est, False, C.byref(m), C.byref(c), None)
            assert rc == 0, rc
        dt = wall(call)
        outputs.append((m.value, bool(c.value), hy.copy()))
        down, calls = E.last_auto_estimation()
        res["auto_host"].append({"route": name, "bytes": n, "seconds": dt, "bytes_per_s": n / dt, "section_bytes_downloaded": down,
                                 "estimator_callbacks": calls, "choice": [m.value, bool(c.value)]})
        print(res["auto_host"][-1], flush=True)

    assert outputs[0][:2] == outputs[1][:2] and np.array_equal(outputs[0][2], outputs[1][2]), "the two routes disagree"
    res["auto_host_routes_agree"] = True
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
