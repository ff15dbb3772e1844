"""The reuse paths of dxtlt_transform_batch_host's pipeline (csrc/batch_host_api.cpp) at a small size.  With the shipped 64 MiB
chunks a pinned arena, a device slot or an event of chunk c - 2 is waited for only from the third chunk on, above 128 MiB.  Here
DXTLT_BATCH_CHUNK_MIB=1 cuts about 11 MiB into ten chunks or more, so every arena and device slot is reused several times per
parity; DXTLT_BATCH_THREADS sets the copy threads per direction.  Both are read when the library loads, so every run is a fresh
child process: it reads the inputs from a file, makes the one call and writes its outputs, guard bytes included, to a second file.
The parent compares them with the oracle (BC1, BC3, BC7) and the CPU statement of the pixel transforms (tests/pixels_ref.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pixels_ref as R
from cabi import BATCH_HOST_ALONE, plan_batch_host

MIB = 1 << 20
GUARD = 32
BLOCK = {"bc1": 8, "bc3": 16, "bc7": 16, "pixels4": 4}
FORMATS = ("bc1", "bc3", "bc7", "pixels4")


def class_bytes(fmt, size_class):
    """the six size classes: empty, one block (pixels4: one pixel), either side of 256 blocks, about 300 KiB, about 700 KiB"""
    B = BLOCK[fmt]
    return (0, B, 255 * B, 257 * B, (300 * 1024 // B + 3) * B, (700 * 1024 // B + 5) * B)[size_class]


_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import dxt_lossless_transform_amd as pkg
from dxt_lossless_transform_amd import batch

specs = json.load(open(sys.argv[2] + ".json"))
inputs = np.load(sys.argv[2])
items, outputs = [], {}
for k, (fmt, inverse, n, settings) in enumerate(specs):
    if fmt == "bc1":
        st = pkg.Bc1TransformSettings(pkg.YCoCgVariant(settings[0]), bool(settings[2]))
    elif fmt == "bc3":
        st = pkg.Bc3TransformSettings(pkg.YCoCgVariant(settings[0]), bool(settings[1]), bool(settings[2]))
    else:
        st = None if fmt == "bc7" else (bool(settings[0]), int(settings[1]))
    y = np.full(n + %d, 0x5A, dtype=np.uint8)
    outputs["y%%d" %% k] = y
    items.append((fmt, bool(inverse), inputs["x%%d" %% k], y[:n], st))
batch.transform_batch_host(items)
np.savez(sys.argv[3], **outputs)
print("done", len(items))
''' % GUARD


def item_specs():
    """(fmt, inverse, bytes, settings) of every item: the size classes under every format and direction, and in their midst one
    item of 1.5 MiB (alone in its chunk at a cap of 1 MiB), one of exactly 2 MiB (goes out alone, through the single-buffer host
    call) and one of 2 MiB less a block (the largest that still travels in a chunk)"""
    specs = []
    for k in range(36):
        fmt, inverse = FORMATS[k % 4], (k // 4) % 2 == 1
        nbytes = class_bytes(fmt, (k + k // 12) % 6)
        settings = (k % 4, (k // 3) % 2, (k // 5) % 2) if fmt in ("bc1", "bc3") else R.SETTINGS[k % len(R.SETTINGS)] if fmt == "pixels4" else None
        specs.append((fmt, inverse, nbytes, settings))
    specs.insert(9, ("bc3", False, 3 * MIB // 2, (1, 1, 1)))
    specs.insert(20, ("bc1", True, 2 * MIB, (2, 0, 1)))
    specs.insert(29, ("bc7", False, 2 * MIB - 16, None))
    return specs


@pytest.fixture(scope="module")
def case(pkg, oracle, tmp_path_factory):
    """the inputs in a file for the children, and what every output must hold: computed once, shared by the runs, left unchanged"""
    specs = item_specs()
    rng = np.random.default_rng(0x5A11)
    inputs, want = {}, []
    for k, (fmt, inverse, n, st) in enumerate(specs):
        raw = rng.integers(0, 256, n, dtype=np.uint8)
        if fmt == "bc7":
            x = oracle.transform_bc7(raw) if inverse and n else raw
            w = oracle.transform_bc7(x, inverse=inverse) if n else raw
        elif fmt == "pixels4":
            x = R.forward(raw, 4, *st) if inverse else raw       # inverse of the statement's forward: the raw pixels again
            w = raw if inverse else R.forward(raw, 4, *st)
        else:
            x = raw
            w = oracle.transform(fmt, x, st[0], bool(st[2]), bool(st[1]), inverse=inverse)
        inputs["x%d" % k] = np.ascontiguousarray(x)
        want.append(np.asarray(w))
    path = str(tmp_path_factory.mktemp("batch_host_small") / "inputs.npz")
    np.savez(path, **inputs)
    json.dump([[fmt, inverse, n, st] for fmt, inverse, n, st in specs], open(path + ".json", "w"))
    return specs, want, path


def test_the_case_reaches_what_it_is_for(pkg):
    """at a cap of 1 MiB (no device needed: the call's own planner): seven chunks or more, a chunk of one item -- fewer than copy
    threads --, the 2 MiB item alone and the one a block shorter in a chunk; every format in both directions, every size class"""
    specs = item_specs()
    lens = [n for _, _, n, _ in specs]
    chunk_of, _, chunks, arena = plan_batch_host(C.CDLL(pkg._lib.lib_path()), lens, MIB)
    assert 36 <= len(specs) <= 44 and 9 * MIB < sum(lens) < 13 * MIB
    assert len(chunks) >= 7 and arena < 3 * MIB
    assert [n for n, c in zip(lens, chunk_of) if c == BATCH_HOST_ALONE] == [2 * MIB]
    for n in (3 * MIB // 2, 2 * MIB - 16):
        assert chunk_of.count(chunk_of[lens.index(n)]) == 1
    assert {(fmt, inverse) for fmt, inverse, _, _ in specs} == {(f, d) for f in FORMATS for d in (False, True)}
    for fmt in FORMATS:
        sizes = sorted({n // BLOCK[fmt] for f, _, n, _ in specs if f == fmt})
        assert sizes[:4] == [0, 1, 255, 257], (fmt, sizes)
        assert any(290 * 1024 < n < 320 * 1024 for f, _, n, _ in specs if f == fmt), fmt
        assert any(690 * 1024 < n < 720 * 1024 for f, _, n, _ in specs if f == fmt), fmt


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_mib,threads", [("1", "3"), (None, "1"), ("1", "1")])
def test_small_host_batch_through_every_reuse_path(case, tmp_path, chunk_mib, threads):
    specs, want, inputs = case
    env = {k: v for k, v in os.environ.items() if k not in ("DXTLT_BATCH_CHUNK_MIB", "DXTLT_BATCH_THREADS")}
    env["DXTLT_BATCH_THREADS"] = threads
    if chunk_mib is not None:
        env["DXTLT_BATCH_CHUNK_MIB"] = chunk_mib
    out = str(tmp_path / "outputs.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, root, inputs, out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "done %d" % len(specs), (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    got = np.load(out)
    for k, (fmt, inverse, n, st) in enumerate(specs):
        y = got["y%d" % k]
        assert y.size == n + GUARD
        assert np.array_equal(y[:n], want[k]), (k, fmt, inverse, n, st)
        assert (y[n:] == 0x5A).all(), (k, fmt, inverse, n)
