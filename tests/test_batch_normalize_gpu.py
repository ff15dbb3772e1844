"""dxtlt_transform_batch_with_normalize_blocks_device on the device, under byte comparison (include/dxtlt_batch_normalize.h; kernels:
csrc/batch_norm_kernels.hip).  Expected bytes are always oracle.transform(fmt, oracle.normalize_bcN_blocks(x, modes), settings)
(batch_normalize_common.expected).  Every call writes into a 0xA5 arena with 256 guard bytes (test_alignment_sweep.GUARD) around
every output; one download per call: every output equals its statement, every other byte still holds the fill, the inputs are
unchanged.  Sizes are in blocks; T is the launch's tile (256 blocks; 512 for BC1 with the colour split).

1. Edges: per format, for the default and the all-off settings, 1, T - 1, T, T + 1, 2T + 9 and 3T blocks at output residues 0
   (aligned form where the size allows it) and 8 (halo form) and input residues 0 and 4, the modes -- both colour modes on BC1 / BC2,
   the 11 pairs on BC3 -- changing from item to item INSIDE one call, so that neighbouring entries of one launch carry different
   modes; every other settings combination once at 2T + 9, residue 8.
2. Lookup forms, read off the plan hook: 303 items of T + 1 blocks (the uniform division), 303 items of 1..5 blocks (one workgroup
   each: the division by one) and the same with one larger item (more than 255 entries in one 4096-workgroup span: the wide
   index), a mixed-size batch of 70 workgroups or more (the bisection past the first 64-workgroup span).
3. Every item of 1 through the single call gives the same bytes.
4. A batch with every mode None gives dxtlt_transform_batch_device's bytes.
5. Items with d_output at residue 1 (launched alone) beside ordinary items.
6. One item per kernel set through dxtlt_transform_batch_device inverse gives normalize_blocks(input).
7. The Python wrapper and the C++ mirror give the C ABI's bytes."""
import os
import subprocess

import numpy as np
import pytest

from batch_normalize_common import (ALL_OFF, BLOCK, DEFAULT, FORMATS, MODE_PAIRS, NORMALIZING, SETTINGS, SINGLE, array, bind, blocks_of, expected,
                                    item, modes_change_the_data, normalized, settings_code, tile_blocks)
from helpers import pkg_settings
from test_alignment_sweep import Arena, dev, device_arena  # noqa: F401
from test_batch_normalize_plan import plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(pkg):
    return bind(pkg)


def counts_of(T):
    return (1, T - 1, T, T + 1, 2 * T + 9, 3 * T)


def edge_entries(fmt):
    """(fmt, settings, modes, blocks, input residue, output residue) of case 1, the modes cycling from item to item"""
    out, pairs = [], MODE_PAIRS[fmt]
    for s in (DEFAULT[fmt], ALL_OFF):
        for n in counts_of(tile_blocks(fmt, s)):
            for p in (0, 8):
                for a in (0, 4):
                    out.append((fmt, s, pairs[len(out) % len(pairs)], n, a, p))
    for s in SETTINGS[fmt]:
        if s not in (DEFAULT[fmt], ALL_OFF):
            out.append((fmt, s, pairs[len(out) % len(pairs)], 2 * tile_blocks(fmt, s) + 9, 4, 8))
    return out


class Placed:
    """entries laid out in one input and one output arena on the device"""

    def __init__(self, oracle, dev, entries, fill=0xA5):
        import torch

        a_in, a_out = Arena(), Arena()
        self.entries = entries
        self.in_at = [a_in.place(a, n * BLOCK[f]) for f, _, _, n, a, _ in entries]
        self.out_at = [a_out.place(p, n * BLOCK[f]) for f, _, _, n, _, p in entries]
        self.h_in = np.zeros(a_in.size(), dtype=np.uint8)
        for (f, _, _, n, _, _), i in zip(entries, self.in_at):
            self.h_in[i:i + n * BLOCK[f]] = blocks_of(oracle, f, n)
        self.d_in = device_arena(dev, self.h_in.size, 0)
        self.d_in.copy_(torch.from_numpy(self.h_in))
        self.fill = fill
        self.d_out = device_arena(dev, a_out.size(), fill)

    def slices(self, k):
        f, _, _, n, _, _ = self.entries[k]
        i, o, nbytes = self.in_at[k], self.out_at[k], n * BLOCK[f]
        return self.d_in[i:i + nbytes], self.d_out[o:o + nbytes]

    def items(self, modes=None):
        out = []
        for k, (f, s, m, n, _, _) in enumerate(self.entries):
            src, dst = self.slices(k)
            out.append(item(f, src.data_ptr(), dst.data_ptr(), n * BLOCK[f], m if modes is None else modes, s))
        return out

    def check(self, wants, label):
        """one download: outputs, guards, inputs"""
        import torch

        torch.cuda.synchronize()
        got = self.d_out.cpu().numpy()
        image = np.full(got.size, self.fill, dtype=np.uint8)
        for o, w in zip(self.out_at, wants):
            image[o:o + w.size] = w
        if not np.array_equal(got, image):
            for k, (o, w) in enumerate(zip(self.out_at, wants)):
                bad = np.nonzero(got[o:o + w.size] != w)[0]
                assert bad.size == 0, f"{label}: item {k} {self.entries[k]}: {bad.size} of {w.size} bytes differ, first at byte {int(bad[0])}"
            stray = np.nonzero(got != image)[0]
            pytest.fail(f"{label}: {stray.size} guard bytes changed, first at arena byte {int(stray[0])}; outputs start at {self.out_at}")
        assert np.array_equal(self.d_in.cpu().numpy(), self.h_in), (label, "the call changed its input")
        return got


def run_call(lib, dev, items):
    import torch

    assert lib.dxtlt_transform_batch_with_normalize_blocks_device(array(items), len(items), torch.cuda.current_stream(dev).cuda_stream) == 0, \
        lib.dxtlt_last_error()


def statement(oracle, entries):
    return [expected(oracle, f, s, n, m) for f, s, m, n, _, _ in entries]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_edges_with_the_modes_mixed_inside_one_call(pkg, oracle, lib, dev, fmt):
    entries = edge_entries(fmt)
    assert {m for _, _, m, _, _, _ in entries} == set(MODE_PAIRS[fmt])
    assert all(a[2] != b[2] for a, b in zip(entries, entries[1:]))
    for f, s, m, n, _, _ in entries:
        assert modes_change_the_data(oracle, f, n, m), (f, n, m)
    placed = Placed(oracle, dev, entries)
    launches, _ = plan(lib, placed.items())
    want_launches = len(SETTINGS[fmt]) if fmt != "bc1" else 2 * 2 + (len(SETTINGS[fmt]) - 2)
    assert [l.kind for l in launches] == [NORMALIZING] * want_launches, [(l.kind, l.settings_code) for l in launches]
    run_call(lib, dev, placed.items())
    placed.check(statement(oracle, entries), f"{fmt} edges")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_lookup_form(pkg, oracle, lib, dev, fmt):
    s = DEFAULT[fmt]
    T = tile_blocks(fmt, s)
    pairs = MODE_PAIRS[fmt] if fmt != "bc1" else MODE_PAIRS[fmt][1:]     # (BC1: one launch holds one mode)
    code = settings_code(fmt, s) | (pairs[0][1] << 8 if fmt == "bc1" else 0)

    def entries_of(counts):
        return [(fmt, s, pairs[k % len(pairs)], n, 4 * (k % 2), 8) for k, n in enumerate(counts)]

    # (`wide` says how the launch's index is built -- 303 entries begin inside one span -- ; only a launch without uniform_wgs reads it)
    small = [1 + k % 5 for k in range(303)]
    mixed = [(1, T + 1, 2 * T + 9, 3 * T)[k % 4] for k in range(40)]
    for label, counts, uniform, wide in (("uniform division", [T + 1] * 303, 2, 1), ("one workgroup each", small, 1, 1),
                                         ("wide index", small + [T + 1], 0, 1), ("bisection", mixed, 0, 0)):
        entries = entries_of(counts)
        placed = Placed(oracle, dev, entries)
        launches, _ = plan(lib, placed.items())
        assert [(l.kind, l.settings_code, l.items, l.uniform_wgs, l.wide) for l in launches] == [(NORMALIZING, code, len(counts), uniform, wide)], label
        assert label != "bisection" or launches[0].workgroups >= 70
        run_call(lib, dev, placed.items())
        placed.check(statement(oracle, entries), f"{fmt} {label}")


def single_call(lib, dev, fmt, src, dst, modes, s):
    """dxtlt_transform_bcN_with_normalize_blocks_device, the C ABI itself"""
    import ctypes as C

    import torch

    vp, sz, u8, b = C.c_void_p, C.c_size_t, C.c_uint8, C.c_bool
    fn = getattr(lib, f"dxtlt_transform_{fmt}_with_normalize_blocks_device")
    fn.argtypes = [vp, vp, sz, u8, u8, u8, b, b, vp] if fmt == "bc3" else [vp, vp, sz, u8, u8, b, vp]
    stream = torch.cuda.current_stream(dev).cuda_stream
    if fmt == "bc3":
        rc = fn(src.data_ptr(), dst.data_ptr(), src.numel(), modes[0], modes[1], s[0], bool(s[1]), bool(s[2]), stream)
    else:
        rc = fn(src.data_ptr(), dst.data_ptr(), src.numel(), modes[1], s[0], bool(s[2]), stream)
    assert rc == 0, lib.dxtlt_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_single_call_gives_the_same_bytes(pkg, oracle, lib, dev, fmt):
    entries = edge_entries(fmt)
    batched, alone = Placed(oracle, dev, entries), Placed(oracle, dev, entries)
    run_call(lib, dev, batched.items())
    for k, (f, s, m, _, _, _) in enumerate(entries):
        src, dst = alone.slices(k)
        single_call(lib, dev, f, src, dst, m, s)
    want = statement(oracle, entries)
    assert np.array_equal(batched.check(want, f"{fmt} batch"), alone.check(want, f"{fmt} single calls"))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_batch_of_none_modes_is_the_plain_batch(pkg, oracle, lib, dev, fmt):
    from dxt_lossless_transform_amd import batch

    entries = [(f, s, (0, 0), n, a, p) for f, s, _, n, a, p in edge_entries(fmt)]
    mine, plain = Placed(oracle, dev, entries), Placed(oracle, dev, entries)
    run_call(lib, dev, mine.items())
    batch.transform_batch([(fmt, False) + plain.slices(k) + (pkg_settings(pkg, fmt, s),) for k, (_, s, _, _, _, _) in enumerate(entries)])
    want = statement(oracle, entries)
    assert np.array_equal(mine.check(want, f"{fmt} all None"), plain.check(want, f"{fmt} plain batch"))


@pytest.mark.gpu
def test_items_that_go_out_alone_sit_beside_ordinary_ones(pkg, oracle, lib, dev):
    entries = []
    for fmt in FORMATS:
        s, m = DEFAULT[fmt], MODE_PAIRS[fmt][-1]
        n = 2 * tile_blocks(fmt, s) + 9
        entries += [(fmt, s, m, n, 0, 8), (fmt, s, m, n, 4, 1), (fmt, s, MODE_PAIRS[fmt][0], n, 0, 0)]
    placed = Placed(oracle, dev, entries)
    launches, _ = plan(lib, placed.items())
    assert [(l.kind, l.first_item) for l in launches if l.kind == SINGLE] == [(SINGLE, 1), (SINGLE, 4), (SINGLE, 7)]
    run_call(lib, dev, placed.items())
    placed.check(statement(oracle, entries), "singles")


@pytest.mark.gpu
def test_the_inverse_batch_yields_the_normalised_blocks(pkg, oracle, lib, dev):
    """one item per kernel set: every settings combination, on BC1 with both colour modes"""
    import torch

    from dxt_lossless_transform_amd import batch

    entries = []
    for fmt in FORMATS:
        for s in SETTINGS[fmt]:
            for m in (MODE_PAIRS[fmt] if fmt == "bc1" else [MODE_PAIRS[fmt][(len(entries)) % len(MODE_PAIRS[fmt])]]):
                entries.append((fmt, s, m, 2 * tile_blocks(fmt, s) + 9, 4, 8))
    assert len(entries) == 16 + 8 + 16
    placed = Placed(oracle, dev, entries)
    run_call(lib, dev, placed.items())
    back = Arena()
    back_at = [back.place(a, n * BLOCK[f]) for f, _, _, n, a, _ in entries]
    d_back = device_arena(dev, back.size(), 0x5A)
    batch.transform_batch([(f, True, placed.slices(k)[1], d_back[o:o + n * BLOCK[f]], pkg_settings(pkg, f, s))
                           for k, ((f, s, _, n, _, _), o) in enumerate(zip(entries, back_at))])
    torch.cuda.synchronize()
    image = np.full(back.size(), 0x5A, dtype=np.uint8)
    for (f, s, m, n, _, _), o in zip(entries, back_at):
        image[o:o + n * BLOCK[f]] = normalized(oracle, f, n, m)
        assert modes_change_the_data(oracle, f, n, m)
    assert np.array_equal(d_back.cpu().numpy(), image)
    placed.check(statement(oracle, entries), "round trip, forward")


@pytest.mark.gpu
def test_the_python_wrapper_gives_the_c_abi_bytes(pkg, oracle, lib, dev):
    from dxt_lossless_transform_amd import batch

    entries = [(fmt, DEFAULT[fmt], MODE_PAIRS[fmt][-1], tile_blocks(fmt, DEFAULT[fmt]) + 1, 0, 8) for fmt in FORMATS]
    c_abi, wrapped = Placed(oracle, dev, entries), Placed(oracle, dev, entries)
    run_call(lib, dev, c_abi.items())
    batch.transform_batch_with_normalize_blocks([(f,) + wrapped.slices(k) + (m, pkg_settings(pkg, f, s)) for k, (f, s, m, _, _, _) in enumerate(entries)])
    batch.transform_batch_with_normalize_blocks([])
    want = statement(oracle, entries)
    assert np.array_equal(c_abi.check(want, "C ABI"), wrapped.check(want, "Python wrapper"))


@pytest.mark.gpu
def test_the_cpp_mirror_gives_the_c_abi_bytes(pkg, oracle, lib, dev, tmp_path):
    """tests/cpp/test_cpp_batch_normalize.cpp: one batch of three items (BC1, BC2, BC3) through dxtlt::transform_batch_with_normalize_blocks_device
    and dxtlt::batch_any_normalizable_device; it writes the three outputs and the flags"""
    libdir = os.path.dirname(pkg._lib.lib_path())
    exe = str(tmp_path / "test_cpp_batch_normalize")
    src = os.path.join(ROOT, "tests", "cpp", "test_cpp_batch_normalize.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, src, f"-L{libdir}", "-ldxtlt_gfx950",
                           "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    entries = [(fmt, DEFAULT[fmt], MODE_PAIRS[fmt][-1], tile_blocks(fmt, DEFAULT[fmt]) + 1, 0, 8) for fmt in FORMATS]
    args = []
    for k, (f, s, m, n, _, _) in enumerate(entries):
        (tmp_path / f"in{k}.bin").write_bytes(blocks_of(oracle, f, n).tobytes())
        args += [f[2], str(tmp_path / f"in{k}.bin"), str(tmp_path / f"out{k}.bin"), str(m[0]), str(m[1]), str(s[0]), str(s[1]), str(s[2])]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["flags", "1", "1", "1"], r.stdout
    placed = Placed(oracle, dev, entries)
    run_call(lib, dev, placed.items())
    got = placed.check(statement(oracle, entries), "C ABI")
    for k, (f, s, m, n, _, _) in enumerate(entries):
        mirror = np.frombuffer((tmp_path / f"out{k}.bin").read_bytes(), dtype=np.uint8)
        o = placed.out_at[k]
        assert np.array_equal(mirror, got[o:o + n * BLOCK[f]]) and np.array_equal(mirror, expected(oracle, f, s, n, m)), f
