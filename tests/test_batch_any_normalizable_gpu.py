"""dxtlt_batch_any_normalizable_device on the device (include/dxtlt_batch_normalize.h; kernel: csrc/batch_norm_kernels.hip): which
items of a batch hold a block that block normalisation would touch.

The CPU statement per item comes from the oracle's normalisers: the flag is 1 when some mode's output differs from the input, or
when the item holds a block that is already in normal form (planted here as the oracle's own output for a block it changes: the
device classification flags such a block, no mode changes it again).  Blocks come from auto_normalize_ref.blocks / class_of, which
generate and label plain, solid and transparent blocks; BC3 items are its 16-byte blocks (random alpha halves) with uniform alpha
halves planted.

One call of more than 300 items, all three formats mixed, inputs at residues 0, 1, 4 and 8:
  * items of 600 blocks (three workgroups) with exactly one flagged block at block 0, 63, 64, 255, 256 and the last one -- the
    lane, wave and workgroup edges -- of every kind (solid colour; BC1 fully transparent; BC3 uniform alpha);
  * items with no flagged block, at every residue;
  * a BC3 block already in normal form, alone among plain blocks;
  * empty items (flag 0, no workgroup);
  * small items of 1..40 blocks of the generator's 'cycle' and 'none' kinds.
d_flags carries 64 guard words on both sides.  A second call on the same d_flags with plain data only returns all zeros: the call
zeroes the flags itself.  The Python wrapper gives the same flags."""
import numpy as np
import pytest

import auto_normalize_ref as R
from batch_normalize_common import BLOCK, FMT_ID, FORMATS, MODE_PAIRS, array, bind, item, normalize
from test_alignment_sweep import Arena, dev, device_arena  # noqa: F401

N = 600
POSITIONS = (0, 63, 64, 255, 256, N - 1)
RESIDUES = (0, 1, 4, 8)
GUARD_WORDS, GUARD_VALUE = 64, 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib(pkg):
    return bind(pkg)


def generated(fmt, kind, n, seed=0):
    """auto_normalize_ref.blocks; BC3 takes the generator's 16-byte blocks: a random alpha half in front of the labelled colour half"""
    x = R.blocks(1 if fmt == "bc1" else 2, kind, n, seed).copy()
    if fmt == "bc3":                                # far-apart alpha endpoints under random indices: no alpha half is uniform by chance
        x.reshape(-1, 16)[:, 0], x.reshape(-1, 16)[:, 1] = 0x10, 0xF0
    return x


def changed_by_some_mode(oracle, fmt, x):
    return any(not np.array_equal(normalize(oracle, fmt, x, m), x) for m in MODE_PAIRS[fmt])


def planted(oracle, fmt, kind, at):
    """N plain blocks with one flagged block at `at`: (blocks, whether the block is in normal form already)"""
    x = generated(fmt, "none", N, seed=at)
    assert not changed_by_some_mode(oracle, fmt, x)
    B = BLOCK[fmt]
    cycle = generated(fmt, "cycle", R.CYCLE)
    block = x[at * B:(at + 1) * B]
    if kind == "solid":
        b = next(b for b in range(R.CYCLE) if R.class_of("cycle", FMT_ID[fmt] if fmt == "bc1" else 2, b) == 2)
        block[B - 8:] = cycle[b * B + B - 8:(b + 1) * B]
    elif kind == "transparent":
        b = next(b for b in range(R.CYCLE) if R.class_of("cycle", 1, b) == 1)
        block[:] = cycle[b * B:(b + 1) * B]
    else:                                           # BC3: a uniform alpha half -- every pixel index 1, the second endpoint's value
        block[:8] = (0x90, 0x80, 0x49, 0x92, 0x24, 0x49, 0x92, 0x24)
        if kind == "normal form":
            block[:] = oracle.normalize_bc3_blocks(block.copy(), 1, 0)
            assert block[0] == 0x80 and not block[1:8].any() and not changed_by_some_mode(oracle, fmt, x)
    if kind != "normal form":
        assert changed_by_some_mode(oracle, fmt, x) and changed_by_some_mode(oracle, fmt, block.copy())
    others = np.delete(x.reshape(-1, B), at, axis=0).reshape(-1)
    assert not changed_by_some_mode(oracle, fmt, others)
    return x, kind == "normal form"


def batch_of(oracle):
    """(fmt, blocks as bytes, input residue, the CPU statement's flag, what it is) of every item"""
    out = []

    def add(fmt, x, flag, what):
        out.append((fmt, x, RESIDUES[len(out) % 4], int(flag), what))

    for fmt in FORMATS:
        for kind in ("solid",) + (("transparent",) if fmt == "bc1" else ()) + (("uniform alpha",) if fmt == "bc3" else ()):
            for at in POSITIONS:
                add(fmt, planted(oracle, fmt, kind, at)[0], 1, f"{kind} block at {at}")
        for r in RESIDUES:
            x = generated(fmt, "none", N, seed=100 + r)
            add(fmt, x, changed_by_some_mode(oracle, fmt, x), "nothing flagged")
        add(fmt, np.zeros(0, dtype=np.uint8), 0, "empty")
    for at in (0, 257, N - 1, 64):
        add("bc3", planted(oracle, "bc3", "normal form", at)[0], 1, f"a block in normal form at {at}")
    k = 0
    while len(out) < 320:
        fmt, kind = FORMATS[k % 3], ("cycle", "none", "none")[(k // 3) % 3]
        x = generated(fmt, kind, 1 + (7 * k) % 40, seed=k)
        add(fmt, x, changed_by_some_mode(oracle, fmt, x), f"{kind}, {x.size // BLOCK[fmt]} blocks")
        k += 1
    return out


def run(lib, dev, batch, d_flags):
    import torch

    arena = Arena()
    at = [arena.place(r, x.size) for _, x, r, _, _ in batch]
    h_in = np.zeros(arena.size(), dtype=np.uint8)
    for (_, x, _, _, _), o in zip(batch, at):
        h_in[o:o + x.size] = x
    d_in = device_arena(dev, h_in.size, 0)
    d_in.copy_(torch.from_numpy(h_in))
    items = [item(fmt, d_in.data_ptr() + o if x.size else 0, 0, x.size, (0, 0), (0, 0, 0)) for (fmt, x, _, _, _), o in zip(batch, at)]
    assert all(it.d_input % 128 == r for it, (_, x, r, _, _) in zip(items, batch) if x.size)
    rc = lib.dxtlt_batch_any_normalizable_device(array(items), len(items), d_flags.data_ptr() + 4 * GUARD_WORDS, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.dxtlt_last_error()
    torch.cuda.synchronize()
    got = d_flags.cpu().numpy().view(np.uint32)
    assert (got[:GUARD_WORDS] == GUARD_VALUE).all() and (got[GUARD_WORDS + len(batch):] == GUARD_VALUE).all(), "a guard word around d_flags changed"
    assert np.array_equal(d_in.cpu().numpy(), h_in), "the call changed its input"
    return got[GUARD_WORDS:GUARD_WORDS + len(batch)], d_in, at


@pytest.mark.gpu
def test_flags_equal_the_cpu_statement(pkg, oracle, lib, dev):
    import torch

    from dxt_lossless_transform_amd import batch as wrappers

    batch = batch_of(oracle)
    assert len(batch) >= 300 and {f for f, *_ in batch} == set(FORMATS) and {r for _, _, r, _, _ in batch} == set(RESIDUES)
    want = np.array([flag for *_, flag, _ in batch], dtype=np.uint32)
    assert 60 < int(want.sum()) < len(batch) - 60
    d_flags = torch.full((len(batch) + 2 * GUARD_WORDS,), GUARD_VALUE, dtype=torch.int32, device=dev)
    got, d_in, at = run(lib, dev, batch, d_flags)
    wrong = [(k, batch[k][0], batch[k][4], f"input residue {batch[k][2]}", int(got[k])) for k in np.nonzero(got != want)[0]]
    assert not wrong, wrong
    # the Python wrapper, on the same inputs
    flags = wrappers.batch_any_normalizable([(fmt, d_in[o:o + x.size]) for (fmt, x, _, _, _), o in zip(batch, at)])
    torch.cuda.synchronize()
    assert np.array_equal(flags.cpu().numpy().view(np.uint32), want)
    # the same flag words again, plain data only: every flag is written, the ones of the first call are gone
    plain = [(fmt, generated(fmt, "none", max(1, x.size // BLOCK[fmt]), seed=7), r, 0, "plain") for fmt, x, r, _, _ in batch]
    assert not any(changed_by_some_mode(oracle, fmt, x) for fmt, x, *_ in plain[:60])
    again, _, _ = run(lib, dev, plain, d_flags)
    assert not again.any(), np.nonzero(again)[0]


@pytest.mark.gpu
def test_defects_and_the_empty_batch(lib, dev):
    import torch

    flags = torch.full((4,), GUARD_VALUE, dtype=torch.int32, device=dev)
    x = torch.zeros(64, dtype=torch.uint8, device=dev)
    good = item("bc3", x.data_ptr(), 0, 64, (0, 0), (0, 0, 0))
    assert lib.dxtlt_batch_any_normalizable_device(None, 0, None, None) == 0
    for bad, status in ((item("bc3", x.data_ptr(), 0, 24, (0, 0), (0, 0, 0)), 1), (item("bc3", 0, 0, 64, (0, 0), (0, 0, 0)), 2)):
        assert lib.dxtlt_batch_any_normalizable_device(array([good, bad]), 2, flags.data_ptr(), None) == status
    bad_format = item("bc3", x.data_ptr(), 0, 64, (0, 0), (0, 0, 0))
    bad_format.format = 4
    assert lib.dxtlt_batch_any_normalizable_device(array([bad_format]), 1, flags.data_ptr(), None) == 2
    assert lib.dxtlt_batch_any_normalizable_device(array([good]), 1, None, None) == 2
    torch.cuda.synchronize()
    assert (flags.cpu().numpy().view(np.uint32) == GUARD_VALUE).all()            # a refused call writes nothing
    # modes and output pointers of an item are not read
    odd = item("bc3", x.data_ptr(), 0, 64, (9, 9), (9, 1, 1))
    assert lib.dxtlt_batch_any_normalizable_device(array([odd]), 1, flags.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert flags.cpu().numpy().view(np.uint32).tolist() == [1, GUARD_VALUE, GUARD_VALUE, GUARD_VALUE]   # zero blocks: uniform alpha, solid colour
