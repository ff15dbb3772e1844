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
    tools/normalize_bench.py bc23-cells --gib G                       one such process: a JSON line with every cell

    tools/normalize_bench.py auto [--mib 1,256,2048] [--processes 3] [--parent-lib PATH] [--out profiles/auto_normalize_bench.json]
        the auto transform with block normalisation (include/dxtlt_auto_normalize.h).  Cells: BC1 / BC2 x fast / all modes x size x
        data ("tenth": about 10 % normalisable blocks, "none": no such block).  Every cell is timed in `processes` fresh processes;
        each times, alternating in rounds, host clock around work that ends in a device synchronise:
          device      dxtlt_transform_bcN_auto_with_normalization_device
          loop        the same work from the calls that existed before it: dxtlt_transform_bcN_with_normalize_blocks_device per
                      candidate with dxtlt_estimate_sizes_device on its colour section, one readback, the winner once more
          plain_auto  dxtlt_transform_bcN_auto_device ("none" data: what the flag-0 path costs on top of it)
          host        the host call with the built-in estimator (sizes up to 256 MiB); host_parent: the same call of the library at
                      --parent-lib (a build of the commit before this call existed on the device: it goes through the callbacks)
        and, with HIP events, the parts of `device`: the candidate kernel, the estimator over its sections, the winner's transform.
    tools/normalize_bench.py auto-cells --mib ... [--parent-lib PATH]   one such process: a JSON line with every cell

    tools/normalize_bench.py auto-bc3 [--mib 1,256,2048] [--processes 3] [--out profiles/auto_normalize_bc3_bench.json]
        the same for BC3 (dxtlt_transform_bc3_auto_with_normalization_device).  `loop` is the same work from the calls that existed
        before it: the 12 / 24 fused dxtlt_transform_bc3_with_normalize_blocks_device launches, one per colour section k (the first
        eight with alpha section k's alpha mode and split), dxtlt_estimate_sizes_device per shown section, one readback, the pick
        over the 96 / 192 sums, the winner once more.  "tenth": every 20th block a solid colour, every 20th a solid by index 1,
        every 20th a uniform alpha half, every 20th an opaque one.
    tools/normalize_bench.py auto-bc3-cells --mib ...                   one such process

    tools/normalize_bench.py batch [--processes 3] [--out profiles/normalize_batch_bench.json]
        the normalising batch call (include/dxtlt_batch_normalize.h).  Cells: shape -- 8000 x 5463 blocks (a mip-chained corpus),
        1024 x 1 MiB, 64 x (16 MiB + 1 block) -- x format and modes: BC1 ReplicateColor, BC2 ReplicateColor, BC3 (3, 2); default
        settings; about 10 % normalisable blocks.  Every cell is timed in `processes` fresh processes; each times, alternating in
        rounds, host clock around work that ends in a device synchronise:
          batch_norm   dxtlt_transform_batch_with_normalize_blocks_device, one call for all items
          loop         the baseline that existed before it: dxtlt_transform_bcN_with_normalize_blocks_device once per item
          plain_batch  the ceiling: dxtlt_transform_batch_device on the same items, no normalisation
        ms per pass over the items and the fraction of the 8 TB/s HBM peak on the algorithmic 2 * len.  Acceptance: in the
        8000-item cells batch_norm is faster than loop in every process by more than the cell's run-to-run spread.
    tools/normalize_bench.py batch-cells                                one such process"""
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


# ---- batch: the normalising batch call -------------------------------------------------------------------------------------------------
BATCH_SHAPES = (("8000 x 5463 blocks", 8000, lambda block: 5463), ("1024 x 1 MiB", 1024, lambda block: (1 << 20) // block),
                ("64 x (16 MiB + 1 block)", 64, lambda block: (16 << 20) // block + 1))
BATCH_FORMATS = ((1, 8, (0, 2), (1, 0, 1)), (2, 16, (0, 2), (1, 0, 1)), (3, 16, (3, 2), (1, 1, 1)))   # format, block, modes, settings


def batch_cells(rounds=5, steps=3):
    """one process of `batch`: every cell's three legs, ms per pass (median / min / max of the rounds)"""
    import ctypes as C
    import statistics
    import time

    from dxt_lossless_transform_amd.batch import DxtltBatchItem, DxtltBatchNormalizeItem

    dev = torch.device("cuda:0")
    lib = C.CDLL(pkg._lib.lib_path())
    vp, sz, u8, b = C.c_void_p, C.c_size_t, C.c_uint8, C.c_bool
    lib.dxtlt_transform_batch_with_normalize_blocks_device.argtypes = [C.POINTER(DxtltBatchNormalizeItem), sz, vp]
    lib.dxtlt_transform_batch_device.argtypes = [C.POINTER(DxtltBatchItem), sz, vp]
    for n in (1, 2):
        getattr(lib, f"dxtlt_transform_bc{n}_with_normalize_blocks_device").argtypes = [vp, vp, sz, u8, u8, b, vp]
    lib.dxtlt_transform_bc3_with_normalize_blocks_device.argtypes = [vp, vp, sz, u8, u8, u8, b, b, vp]
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    for shape, count, blocks_of in BATCH_SHAPES:
        for fmt, block, (am, cm), (v, sa, sc) in BATCH_FORMATS:
            nbytes = blocks_of(block) * block
            pitch = (nbytes + 255) & ~255
            x = torch.empty(count * pitch, dtype=torch.uint8, device=dev)
            pkg.fill_splitmix64(x, 0xBA7C0000 + fmt)
            y = torch.empty_like(x)
            # about 10 % normalisable blocks: every 10th a solid colour (BC3: every 20th, and every 20th an opaque alpha half)
            if pitch == nbytes:
                every = [x.view(-1, block)]
            else:
                every = [x[k * pitch:k * pitch + nbytes].view(-1, block) for k in range(count)]
            for rows in every:
                if fmt == 3:
                    rows[0::20, 12:] = 0
                    rows[10::20, 0:2] = 0xFF
                else:
                    rows[0::10, block - 4:] = 0
            norm_items, plain_items, singles = (DxtltBatchNormalizeItem * count)(), (DxtltBatchItem * count)(), []
            for k in range(count):
                src, dst = x.data_ptr() + k * pitch, y.data_ptr() + k * pitch
                norm_items[k] = DxtltBatchNormalizeItem(src, dst, nbytes, fmt, am, cm, v, sa, sc)
                plain_items[k] = DxtltBatchItem(src, dst, nbytes, fmt, 0, v, sa, sc)
                singles.append((src, dst, nbytes, am, cm, v, bool(sa), bool(sc), stream) if fmt == 3 else (src, dst, nbytes, cm, v, bool(sc), stream))
            single = getattr(lib, f"dxtlt_transform_bc{fmt}_with_normalize_blocks_device")

            def loop():
                for args in singles:
                    if single(*args) != 0:
                        raise RuntimeError("single fused call failed")

            def batch_norm():
                if lib.dxtlt_transform_batch_with_normalize_blocks_device(norm_items, count, stream) != 0:
                    raise RuntimeError("normalising batch call failed")

            def plain_batch():
                if lib.dxtlt_transform_batch_device(plain_items, count, stream) != 0:
                    raise RuntimeError("plain batch call failed")

            legs = {"batch_norm": batch_norm, "loop": loop, "plain_batch": plain_batch}
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.1:   # warm up by wall time (clock ramp), every leg
                for fn in legs.values():
                    fn()
                torch.cuda.synchronize()
            ms = {k: [] for k in legs}
            for _ in range(rounds):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        fn()
                    torch.cuda.synchronize()
                    ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
            cell = f"bc{fmt} modes=({am}, {cm}) {shape}"
            out[cell] = {k: {"ms": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                             "of_peak_on_2len": round(2 * count * nbytes / (statistics.median(t) * 1e-3) / 8e12, 4)} for k, t in ms.items()}
            del x, y, every
            torch.cuda.empty_cache()
    return out


def batch_main(argv):
    import argparse
    import subprocess

    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "normalize_batch_bench.json"))
    a = ap.parse_args(argv)
    runs = []
    for _ in range(a.processes):   # one after the other: fresh processes, never two on the device at once
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "batch-cells"], capture_output=True, text=True, check=True)
        runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
    cells, accepted = {}, True
    for cell in runs[0]:
        legs = {k: [r[cell][k] for r in runs] for k in ("batch_norm", "loop", "plain_batch")}
        spread = max(max(p["ms"] for p in v) - min(p["ms"] for p in v) for v in legs.values())
        margins = [round(l["ms"] - n["ms"], 4) for n, l in zip(legs["batch_norm"], legs["loop"])]
        ok = all(m > spread for m in margins)
        if "8000 x" in cell:
            accepted = accepted and ok
        cells[cell] = {"processes": legs, "spread_ms": round(spread, 4), "loop_minus_batch_norm_ms": margins,
                       "batch_norm_over_plain_batch": [round(n["ms"] / p["ms"], 4) for n, p in zip(legs["batch_norm"], legs["plain_batch"])],
                       "batch_norm_faster_than_loop_by_more_than_the_spread": ok}
    res = {"workload": "forward transform with fused block normalisation of many device buffers: BC1 ReplicateColor, BC2 ReplicateColor, "
                       "BC3 (OpaqueZeroAlphaMaxIndices, ReplicateColor); default settings; about 10 % normalisable blocks",
           "legs": "ms per pass over all items, host clock around 3 passes and a device synchronise, median / min / max of 5 rounds, the "
                   "three legs alternating; of_peak_on_2len: 2 * len of all items / ms / 8 TB/s",
           "acceptance": "the 8000-item cells: batch_norm faster than loop in every process by more than the spread",
           "processes_per_cell": a.processes, "accepted": accepted, "cells": cells}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"accepted": accepted, "out": a.out, "cells": len(cells)}))


# ---- auto: the auto transform with block normalisation ---------------------------------------------------------------------------------
def auto_data(fmt, nbytes, kind, dev):
    """random blocks none of which any mode changes (c0 != c1, pixels 0 and 1 with different indices); "tenth": every 20th block a solid
    colour by index 0 and every 20th a fully transparent block (BC1) / a solid by index 1 (BC2)"""
    bb, at = (8, 0) if fmt == 1 else (16, 8)
    n = nbytes // bb
    if fmt == 3:
        return auto_data_bc3(n, kind, dev)
    x = torch.empty(n * bb, dtype=torch.uint8, device=dev)
    pkg.fill_splitmix64(x, 0xA0700 + fmt)
    b = x.view(-1, bb)
    for lo in range(0, n, 1 << 24):
        v = b[lo:min(n, lo + (1 << 24))]
        v[:, at] |= 1
        v[:, at + 2] &= 0xFE
        v[:, at + 4] = (v[:, at + 4] & 0xF0) | 4
    if kind == "tenth":
        b[0::20, at + 4:at + 8] = 0
        if fmt == 1:
            b[10::20, at:at + 2] = 0
            b[10::20, at + 4:at + 8] = 0xFF
        else:
            b[10::20, at + 4:at + 8] = 0x55
    return x


def auto_data_bc3(n, kind, dev):
    """BC2's colour halves behind alpha halves no alpha mode changes (a0 >= 128 > 119 >= a1, pixels 0 and 1 with indices 0 and 1);
    "tenth": every 20th block a uniform alpha half by index 0 and every 20th an opaque one, (255, a1) by index 0"""
    x = auto_data(2, n * 16, kind, dev)
    b = x.view(-1, 16)
    for lo in range(0, n, 1 << 24):
        v = b[lo:min(n, lo + (1 << 24))]
        v[:, 0] |= 0x80
        v[:, 1] &= 0x77
        v[:, 2] = (v[:, 2] & 0xC0) | 0x08
    if kind == "tenth":
        b[5::20, 2:8] = 0
        b[15::20, 2:8] = 0
        b[15::20, 0] = 0xFF
    return x


# the test orders: BC1 / BC2 (variant, split colour), BC3 (variant, split alpha, split colour)
AUTO_FAST = [(0, 0), (0, 1), (1, 0), (1, 1)]
AUTO_ALL = [(2, 0), (0, 0), (0, 1), (3, 0), (3, 1), (2, 1), (1, 0), (1, 1)]
AUTO_FAST3 = [(1, 1, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1), (0, 0, 0), (1, 0, 0)]
AUTO_ALL3 = [(2, 1, 0), (2, 1, 1), (3, 1, 1), (3, 1, 0), (1, 1, 0), (3, 0, 1), (1, 1, 1), (2, 0, 1),
             (2, 0, 0), (3, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1), (0, 0, 0), (1, 0, 0)]


def auto_plan(fmt, use_all, nbytes, y_ptr):
    """What the legs of auto_cells need to know about (format, depth), so that they are written once:
      launches       the fused launches of the `loop` leg: (settings of dxtlt_transform_bcN_with_normalize_blocks_device behind
                     `len`, [((address, length) of a section of the output to estimate after it, its counter)])
      cands          the candidates in the order they are compared: (settings, the counters its total is the sum of)
      section_lens   the candidate arena, end to end, in counter order
      mode_outs      how many of the call's out-parameters are uint8 modes (the rest are bool splits); the plain auto call takes
                     the last of them and the splits
    BC1 / BC2: one launch, one colour section and one counter per candidate.  BC3: one launch per colour section k (counter 8 + k),
    the first eight with alpha section k's mode and split (counter k); a candidate is alpha counter + colour counter."""
    variants = 4 if use_all else 2
    blocks = nbytes // (8 if fmt == 1 else 16)
    colour = (y_ptr, nbytes // 2) if fmt == 1 else (y_ptr + nbytes // 2, nbytes // 4)
    if fmt != 3:
        settings = [(norm, v, bool(sc)) for norm in range(3) for v, sc in (AUTO_ALL if use_all else AUTO_FAST)]
        return {"launches": [(st, [(colour, i)]) for i, st in enumerate(settings)], "cands": [(st, (i,)) for i, st in enumerate(settings)],
                "section_lens": [4 * blocks] * len(settings), "mode_outs": 2}
    alpha = (y_ptr, 2 * blocks)
    launches = []
    for k in range(6 * variants):
        am, sa = (k // 2, k % 2) if k < 8 else (0, 0)
        st = (am, k // (2 * variants), k // 2 % variants, bool(sa), bool(k % 2))
        launches.append((st, [(colour, 8 + k)] + ([(alpha, k)] if k < 8 else [])))
    cands = [((am, cm, v, bool(sa), bool(sc)), (2 * am + sa, 8 + cm * 2 * variants + 2 * v + sc))
             for am in range(4) for cm in range(3) for v, sa, sc in (AUTO_ALL3 if use_all else AUTO_FAST3)]
    return {"launches": launches, "cands": cands, "section_lens": [2 * blocks] * 8 + [4 * blocks] * (6 * variants), "mode_outs": 3}


def auto_cells(mibs, parent_lib=None, rounds=3, fmts=(1, 2)):
    import ctypes as C
    import statistics
    import time

    lib = C.CDLL(pkg._lib.lib_path())
    parent = C.CDLL(parent_lib) if parent_lib else None
    vp, sz, u8, b, u8p, bp, u64p = C.c_void_p, C.c_size_t, C.c_uint8, C.c_bool, C.POINTER(C.c_uint8), C.POINTER(C.c_bool), C.POINTER(C.c_uint64)

    class Sec(C.Structure):
        _fields_ = [("d_ptr", vp), ("len", C.c_uint64)]

    for l in (lib, parent):
        if l is None:
            continue
        l.dxtlt_builtin_size_estimator.restype = vp
        l.dxtlt_transform_bc1_auto_with_normalization.argtypes = [vp, vp, sz, vp, b, u8p, u8p, bp, C.POINTER(C.c_uint32)]
    for n in fmts:
        outs = [u8p, u8p, u8p, bp, bp] if n == 3 else [u8p, u8p, bp]
        getattr(lib, f"dxtlt_transform_bc{n}_auto_with_normalization_device").argtypes = [vp, vp, sz, b, vp] + outs
        getattr(lib, f"dxtlt_transform_bc{n}_auto_with_normalization").argtypes = [vp, vp, sz, vp, b] + outs + [C.POINTER(C.c_uint32)]
        getattr(lib, f"dxtlt_transform_bc{n}_auto_device").argtypes = [vp, vp, sz, b, vp] + outs[-3 if n == 3 else -2:]
        getattr(lib, f"dxtlt_transform_bc{n}_with_normalize_blocks_device").argtypes = [vp, vp, sz] + ([u8, u8, u8, b, b] if n == 3 else [u8, u8, b]) + [vp]
    lib.dxtlt_estimate_sizes_device.argtypes = [C.POINTER(Sec), sz, vp, vp]
    lib.dxtlt_debug_auto_normalization_candidates_into_device.argtypes = [C.c_int32, b, vp, sz, vp, C.c_uint64, vp]
    if 3 in fmts:
        lib.dxtlt_debug_bc3_auto_normalization_candidates_into_device.argtypes = [b, vp, sz, vp, C.c_uint64, vp]
    lib.dxtlt_debug_auto_normalization_last.argtypes = [u64p]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    out = {}

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"status {rc}")

    def wall_ms(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for mib in mibs:
        nbytes = int(mib * (1 << 20))
        steps = 20 if mib <= 16 else 3
        for fmt in fmts:
            for kind in ("tenth", "none"):
                x = auto_data(fmt, nbytes, kind, dev)
                y = torch.empty_like(x)
                for use_all in (False, True):
                    plan = auto_plan(fmt, use_all, nbytes, y.data_ptr())
                    cands, lens = plan["cands"], plan["section_lens"]
                    sizes = torch.zeros(len(lens), dtype=torch.int64, device=dev)
                    choice = [u8() for _ in range(plan["mode_outs"])] + [b() for _ in range(len(cands[0][0]) - plan["mode_outs"])]
                    refs = [C.byref(c) for c in choice]
                    fused = getattr(lib, f"dxtlt_transform_bc{fmt}_with_normalize_blocks_device")

                    def device():
                        ok(getattr(lib, f"dxtlt_transform_bc{fmt}_auto_with_normalization_device")(x.data_ptr(), y.data_ptr(), nbytes, use_all, stream, *refs))

                    def loop():
                        for settings, shown in plan["launches"]:
                            ok(fused(x.data_ptr(), y.data_ptr(), nbytes, *settings, stream))
                            for (at, length), counter in shown:
                                ok(lib.dxtlt_estimate_sizes_device(C.byref(Sec(at, length)), 1, stream, sizes.data_ptr() + 8 * counter))
                        got = sizes.cpu().tolist()                       # the one readback
                        totals = [sum(got[c] for c in counters) for _settings, counters in cands]
                        ok(fused(x.data_ptr(), y.data_ptr(), nbytes, *cands[totals.index(min(totals))][0], stream))

                    def plain_auto():
                        ok(getattr(lib, f"dxtlt_transform_bc{fmt}_auto_device")(x.data_ptr(), y.data_ptr(), nbytes, use_all, stream, *refs[plan["mode_outs"] - 1:]))

                    legs = {"device": device, "loop": loop, "plain_auto": plain_auto}
                    if mib <= 256:
                        hx = x.cpu().numpy()
                        hy = hx.copy()

                        def host(l=lib):
                            f = getattr(l, f"dxtlt_transform_bc{fmt}_auto_with_normalization")
                            ok(f(hx.ctypes.data, hy.ctypes.data, nbytes, l.dxtlt_builtin_size_estimator(), use_all, *refs, None))

                        legs["host"] = host
                        if parent is not None and fmt == 1:
                            legs["host_parent"] = lambda: host(parent)
                    for fn in legs.values():                             # warm up every leg: code objects, arenas, staging buffers
                        fn()
                        torch.cuda.synchronize()
                    device()
                    last = (C.c_uint64 * 4)()
                    lib.dxtlt_debug_auto_normalization_last(last)
                    picked = [int(c.value) for c in choice]
                    ms = {k: [] for k in legs}
                    for _ in range(rounds):
                        for k, fn in legs.items():
                            ms[k].append(wall_ms(fn, 1 if k.startswith("host") and mib > 16 else steps))
                    cell = {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()}
                    cell["flag"], cell["choice"] = int(last[3]), picked
                    if kind == "tenth":                                  # the parts of `device`, HIP events
                        arena = torch.empty(sum(lens), dtype=torch.uint8, device=dev)
                        secs = (Sec * len(lens))(*[Sec(arena.data_ptr() + sum(lens[:k]), lens[k]) for k in range(len(lens))])
                        winner = picked[:plan["mode_outs"]] + [bool(v) for v in picked[plan["mode_outs"]:]]
                        if fmt == 3:
                            hook = lambda *a: lib.dxtlt_debug_bc3_auto_normalization_candidates_into_device(use_all, *a)
                        else:
                            hook = lambda *a: lib.dxtlt_debug_auto_normalization_candidates_into_device(fmt, use_all, *a)
                        parts = {
                            "candidates": lambda: ok(hook(x.data_ptr(), nbytes, arena.data_ptr(), arena.numel(), stream)),
                            "estimator": lambda: ok(lib.dxtlt_estimate_sizes_device(secs, len(lens), stream, sizes.data_ptr())),
                            "winner": lambda: ok(fused(x.data_ptr(), y.data_ptr(), nbytes, *winner, stream)),
                        }
                        for fn in parts.values():
                            fn()
                        cell["parts_event_ms"] = {k: round(statistics.median([event_ms(fn, steps) for _ in range(rounds)]), 4) for k, fn in parts.items()}
                        del arena
                    out[f"bc{fmt} {'all' if use_all else 'fast'} {mib:g}MiB {kind}"] = cell
                del x, y
                torch.cuda.empty_cache()
    return out


def auto_main(argv, bc3=False):
    import argparse
    import subprocess

    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="1,256,2048")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "auto_normalize_bc3_bench.json" if bc3 else "auto_normalize_bench.json"))
    a = ap.parse_args(argv)
    runs = []
    for _ in range(a.processes):   # one after the other: fresh processes, never two on the device at once
        cmd = [sys.executable, os.path.abspath(__file__), "auto-bc3-cells" if bc3 else "auto-cells", "--mib", a.mib] + (["--parent-lib", a.parent_lib] if a.parent_lib else [])
        done = subprocess.run(cmd, capture_output=True, text=True, check=True)
        runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(f"process {len(runs)} of {a.processes} done", file=sys.stderr, flush=True)
    cells, all_faster = {}, True
    for name in runs[0]:
        legs = {k: [r[name][k] for r in runs] for k in runs[0][name] if isinstance(runs[0][name][k], dict) and "ms" in runs[0][name][k]}
        spread = max(max(p["ms"] for p in legs[k]) - min(p["ms"] for p in legs[k]) for k in ("device", "loop"))   # of the two legs compared
        margins = [round(l["ms"] - d["ms"], 4) for d, l in zip(legs["device"], legs["loop"])]
        faster = all(m > spread for m in margins)
        cell = {"processes": legs, "spread_ms": round(spread, 4), "loop_minus_device_ms": margins,
                "loop_over_device": [round(l["ms"] / d["ms"], 3) for d, l in zip(legs["device"], legs["loop"])],
                "device_faster_than_loop_by_more_than_the_spread": faster, "flag": runs[0][name]["flag"], "choice": runs[0][name]["choice"]}
        if name.endswith("none"):
            cell["device_minus_plain_auto_ms"] = [round(d["ms"] - p["ms"], 4) for d, p in zip(legs["device"], legs["plain_auto"])]
        else:
            all_faster = all_faster and faster
        if "host_parent" in legs:
            cell["host_parent_over_host"] = [round(p["ms"] / h["ms"], 3) for h, p in zip(legs["host"], legs["host_parent"])]
        if "parts_event_ms" in runs[0][name]:
            parts = [r[name]["parts_event_ms"] for r in runs]
            cell["parts_event_ms"] = parts
            cell["estimator_share_of_device"] = [round(p["estimator"] / d["ms"], 3) for p, d in zip(parts, legs["device"])]
        cells[name] = cell
    tenth = "10 % normalisable colour halves and 10 % normalisable alpha halves (20 % of blocks)" if bc3 else "about 10 % normalisable blocks"
    res = {"workload": f"auto transform with block normalisation, {'BC3' if bc3 else 'BC1 / BC2'}, fast / all modes; 'tenth': {tenth}, 'none': no such block",
           "legs": "ms per call, host clock around work that ends in a device synchronise; median / min / max of 3 rounds, the legs alternating; "
                   f"parts_event_ms: HIP events around the candidate kernel, the estimator over its {'20 / 32' if bc3 else '12 / 24'} sections and the winner's transform",
           "spread_ms": "the larger max - min over the processes of the device and the loop leg's ms",
           "processes_per_cell": a.processes, "parent_lib_measured": bool(a.parent_lib),
           "device_faster_than_loop_in_every_tenth_cell": all_faster, "cells": cells}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "cells": len(cells), "device_faster_than_loop_in_every_tenth_cell": all_faster}))


if len(sys.argv) > 1 and sys.argv[1] == "auto-cells":
    _mibs = [float(v) for v in sys.argv[sys.argv.index("--mib") + 1].split(",")]
    print(json.dumps(auto_cells(_mibs, sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None)))
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "auto":
    auto_main(sys.argv[2:])
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "auto-bc3-cells":
    print(json.dumps(auto_cells([float(v) for v in sys.argv[sys.argv.index("--mib") + 1].split(",")], fmts=(3,))))
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "auto-bc3":
    auto_main(sys.argv[2:], bc3=True)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "batch-cells":
    print(json.dumps(batch_cells()))
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "batch":
    batch_main(sys.argv[2:])
    sys.exit(0)
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
