#!/usr/bin/env python3
"""The built-in size estimator (docs/ESTIMATOR.md) as a chooser, on the CPU: for the reference's three 256 x 256 test textures
(tests/golden/r2-256-bc{1,2,3}.payload.bin) and all 8 / 8 / 16 candidates of the auto transform, the estimate of the section(s)
the auto transform shows its estimator, the zlib-6 size of the whole transformed buffer, and which candidate the estimator picks
(the reference's order, strict `<`) -- next to the pick of a zlib-1-length estimator.  `--sweep` repeats the picks for other
window sizes W and table sizes BITS (the one tuning the definition allows before the kernel is frozen).

    python tools/estimator_lab.py [--sweep] [--markdown]

Uses the CPU statements in tests/estimator_ref.py and the C oracle; no GPU."""
import argparse
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import estimator_ref as R  # noqa: E402
from oracle import oracle_auto, oracle_c  # noqa: E402


def shown(fmt, n):
    blocks = n // oracle_c.BLOCK[fmt]
    return {"bc1": [(0, n // 2)], "bc2": [(n // 2, n // 4)], "bc3": [(0, blocks * 2), (n // 2, blocks * 4)]}[fmt]


def table(fmt, estimate):
    data = np.fromfile(os.path.join(ROOT, "tests", "golden", f"r2-256-{fmt}.payload.bin"), dtype=np.uint8)
    rows = []
    for v, sa, sc in oracle_auto.test_order(fmt, True):
        out = np.asarray(oracle_c.transform(fmt, data, v, sc, sa))
        secs = [out[o:o + ln] for o, ln in shown(fmt, data.size)]
        rows.append(dict(cand=(v, sa, sc), est=sum(estimate(s) for s in secs), z1=sum(len(zlib.compress(s.tobytes(), 1)) for s in secs),
                         z6=len(zlib.compress(out.tobytes(), 6))))
    return rows


def pick(rows, key):
    best = None
    for r in rows:
        if best is None or r[key] < best[key]:
            best = r
    return best


def summary(rows):
    z6 = [r["z6"] for r in rows]
    lo, hi = min(z6), max(z6)
    return lo, hi, pick(rows, "est"), pick(rows, "z1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    for fmt in ("bc1", "bc2", "bc3"):
        rows = table(fmt, R.estimate)
        lo, hi, p, pz = summary(rows)
        if args.markdown:
            print(f"\n**{fmt.upper()}** (`r2-256-{fmt}`, {len(rows)} candidates; variant, split alpha, split colour)\n")
            print("| candidate | estimate | zlib-1 of the section(s) | zlib-6 of the buffer | above the best |")
            print("|---|---|---|---|---|")
            for r in rows:
                marks = (" **pick**" if r is p else "") + (" *(zlib-1 pick)*" if r is pz else "")
                print(f"| {r['cand']}{marks} | {r['est']} | {r['z1']} | {r['z6']} | {100 * (r['z6'] / lo - 1):.2f} % |")
        else:
            for r in rows:
                print(fmt, r["cand"], r["est"], r["z1"], r["z6"], "<- pick" if r is p else "", "<- zlib-1 pick" if r is pz else "")
        print(f"\n{fmt}: pick {p['cand']} is {100 * (p['z6'] / lo - 1):.2f} % above the best candidate, the worst is {100 * (hi / lo - 1):.2f} % above it; "
              f"the zlib-1 pick {pz['cand']} is {100 * (pz['z6'] / lo - 1):.2f} % above it")
        assert p["z6"] < hi
    if args.sweep:
        print("\n| W | BITS | LDS (window + table) | BC1 pick above best | BC2 | BC3 |" if args.markdown else "\nW BITS lds bc1 bc2 bc3")
        if args.markdown:
            print("|---|---|---|---|---|---|")
        for w, bits in ((32768, 14), (32768, 13), (16384, 14), (16384, 13), (16384, 12), (8192, 13), (8192, 12), (8192, 11), (4096, 11)):
            cells = []
            for fmt in ("bc1", "bc2", "bc3"):
                rows = table(fmt, lambda s, w=w, bits=bits: R.estimate(s, w, bits))
                lo, hi, p, _ = summary(rows)
                cells.append(f"{100 * (p['z6'] / lo - 1):.2f} %")
            lds = f"{(w + (4 << bits)) // 1024} KiB"
            print(f"| {w} | {bits} | {lds} | " + " | ".join(cells) + " |" if args.markdown else f"{w} {bits} {lds} " + " ".join(cells))


if __name__ == "__main__":
    main()
