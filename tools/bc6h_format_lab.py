#!/usr/bin/env python3
"""Candidate record layouts of the BC6H transform (docs/BC6H_FORMAT.md section 4) under zlib-6 and zstd-3 -- CPU only.

    python tools/bc6h_format_lab.py [path/to/r2-256.png]

Corpora: the smooth HDR texture lifted from r2-256.png and encoded by tools/bc6h_synth.py, and a seeded mode-mixed random
corpus (the control).  Candidates (tests/bc6h_ref.py `variant`): a = granule sort only, bytes in block order; b = field split,
endpoints whole; c = b + the high byte of every base endpoint of 8 bits or more at the top of the record; d = c + red and blue
as differences to green.  Prints one JSON line: per corpus the untransformed sizes and each candidate's size relative to them.
"""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bc6h_ref as R  # noqa: E402
import bc6h_synth  # noqa: E402
from tools import zstd_ratio  # noqa: E402

DEFAULT_PNG = "/root/reference/src/assets/tests/r2-256.png"


def sizes(b: bytes) -> dict:
    out = {"zlib6": len(zlib.compress(b, 6))}
    if zstd_ratio.available():
        out["zstd3"] = zstd_ratio.compressed_size(b, 3)
    return out


def main() -> None:
    png = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_PNG
    corpora = {}
    if os.path.exists(png):
        corpora["smooth_hdr"] = bc6h_synth.encode(bc6h_synth.hdr_from_png(png))
    corpora["random_modes"] = bc6h_synth.random_blocks(16384, 0xBC6)
    result = {}
    for name, blocks in corpora.items():
        raw = blocks.reshape(-1)
        base = sizes(raw.tobytes())
        counts = np.bincount(R.block_class(blocks[:, 0]), minlength=R.CLASSES).tolist()
        row = {"blocks": int(blocks.shape[0]), "class_counts": counts, "untransformed": base}
        for v in "abcd":
            t = R.transform(raw, v)
            assert np.array_equal(R.untransform(t, v), raw), v
            s = sizes(t.tobytes())
            row[v] = {k: round(s[k] / base[k] - 1.0, 4) for k in s}
        result[name] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
