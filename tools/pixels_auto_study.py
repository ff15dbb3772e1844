#!/usr/bin/env python3
"""Which estimator ranks the six pixel settings (docs/PIXEL_FORMAT.md) the way a compressor does -- CPU only, no library, no GPU.

The data sets of tools/pixels_gain.py (the r2-256 image comes from tests/golden/r2-256-bc7.payload.bin through
tests/bc7_decode_ref.py, so nothing outside the repository is read) and two sets of independent bounded random walks.  Per data set
and setting, in the candidate order of the pixel auto transform: zlib-6, zstd-3 (system libzstd through tools/zstd_ratio.py, null
without it), the entropy estimate (tests/entropy_ref.py) and the gram estimate (tests/estimator_ref.py) of the setting's whole
output; and each column's pick (first smallest).
    python tools/pixels_auto_study.py > profiles/pixels_auto_study.json"""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import entropy_ref  # noqa: E402
import estimator_ref  # noqa: E402
import pixels_auto_data  # noqa: E402
import pixels_ref  # noqa: E402
from tools import zstd_ratio  # noqa: E402
from tools.pixels_gain import LAYOUT_NAMES  # noqa: E402


def study(name, px):
    B, flat = px.shape[1], np.ascontiguousarray(px).reshape(-1)
    rows = []
    for decorrelate, layout in entropy_ref.CANDIDATES:
        t = pixels_ref.forward(flat, B, decorrelate, layout)
        rows.append({"decorrelate": decorrelate, "layout": LAYOUT_NAMES[layout], "zlib6": len(zlib.compress(t.tobytes(), 6)),
                     "zstd3": zstd_ratio.compressed_size(t.tobytes(), 3) if zstd_ratio.available() else None,
                     "entropy": entropy_ref.estimate(t), "gram": estimator_ref.estimate(t)})
    picks = {k: entropy_ref.pick([r[k] for r in rows]) + 1 for k in ("zlib6", "zstd3", "entropy", "gram") if rows[0][k] is not None}
    return {"data": name, "pixel_bytes": B, "pixels": int(px.shape[0]), "settings": rows, "pick_1_based": picks}


def main():
    rows = [study(name, px) for name, px, _want in pixels_auto_data.data_sets()]
    print(json.dumps({"tool": "pixels_auto_study", "zstd_version": zstd_ratio.version(), "entropy_estimator_version": entropy_ref.VERSION,
                      "gram_estimator_version": estimator_ref.VERSION, "rows": rows}))


if __name__ == "__main__":
    main()
