"""The granule sort of BC7 and BC6H (csrc/granule_sort.h) on chosen class arrangements (tests/granule_patterns.py) and at every
tail length.

CPU lane (no GPU): every layout through the CPU statements of both formats, and a check written from the format documents that
uses neither statement's sort -- it pins the expected bytes before any kernel sees them.  GPU lane: the same layouts and every
tail length 1..1023 through every entry point that reaches the sort (device call, range call, host call, sharded call, batch
call), forward against the CPU statement byte for byte, the inverse of the CPU statement's output against the input, guard
bytes around every output."""
import numpy as np
import pytest

import bc6h_ref as R
import granule_patterns as P
from oracle import oracle_np as onp

FORMATS = ("bc7", "bc6h")
G = P.GRANULE
STREAMS = ((0, 8, 1), (8, 2, 9), (10, 1, 11), (11, 1, 12), (12, 1, 13), (13, 1, 14), (14, 1, 15))   # (offset, width, record byte)
CASES = [(fmt, name) for fmt in FORMATS for name in P.layout_names(P.CLASSES[fmt])]
GUARD = 64


def forward(fmt, oracle, x):
    return oracle.transform_bc7(x) if fmt == "bc7" else R.transform(x)


def inverse(fmt, oracle, y):
    return oracle.transform_bc7(y, inverse=True) if fmt == "bc7" else R.untransform(y)


def records(fmt, oracle, x):
    if fmt == "bc7":
        return np.stack([oracle.bc7_record(x[16 * i:16 * i + 16]) for i in range(x.size // 16)])
    return R.records(x.reshape(-1, 16))


def check_by_hand(cls, recs, y):
    """docs/BC7_FORMAT.md, docs/BC6H_FORMAT.md: the first n - n % 1024 blocks and the rest are two parts, each with its own
    streams; F (record byte 0) in block order; inside each granule the other record bytes in stable class order"""
    n = cls.size
    main = n - n % G
    for start, m in ((0, main), (main, n - main)):
        if m == 0:
            continue
        part, rec = y[16 * start:16 * (start + m)], recs[start:start + m]
        assert np.array_equal(part[15 * m:], rec[:, 0])
        for g0 in range(0, m, G):
            k = min(G, m - g0)
            order = g0 + np.argsort(cls[start + g0:start + g0 + k], kind="stable")
            for off, w, rb in STREAMS:
                assert np.array_equal(part[off * m + w * g0:off * m + w * (g0 + k)].reshape(k, w), rec[order][:, rb:rb + w]), (start, g0, off)


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_layouts_hold_the_edge_values_they_are_named_for():
    for classes in (9, 15):
        lay = dict(P.class_layouts(classes))
        last = classes - 1
        per_segment = lambda a, c: (a.reshape(-1, 64) == c).sum(axis=1)
        assert set(per_segment(lay["segment_pure"], 0).tolist()) == {0, 64}
        assert not np.array_equal(lay["segment_pure"][:G], lay["segment_pure"][G:])
        assert (np.diff(lay["descending"]) <= 0).all() and (np.diff(lay["ascending"]) >= 0).all()
        assert all((per_segment(lay["round_robin"], c) > 0).all() for c in range(classes))
        for p in P.STRANGER_POSITIONS:
            a, b = lay[f"one_stranger_p{p}"], lay[f"reserved_with_stranger_p{p}"]
            assert a[p] == last and (a == last).sum() == 1 and np.unique(a).size == 2
            assert b[p] == 0 and (b == last).sum() == G - 1
        assert (lay["all_reserved"] == last).all()
        for name in ("exact_1023_plus_1_sorts_first", "exact_1023_plus_1_sorts_last"):
            assert sorted(np.bincount(lay[name], minlength=classes).tolist())[-2:] == [1, 1023]
        for name in ("exact_512_512_even_odd", "exact_512_512_odd_even"):
            a = lay[name]
            c0, c1 = a[0], a[64]
            assert (a == c0).sum() == 512 and (a == c1).sum() == 512
            assert per_segment(a, c0).tolist() == [64, 0] * 8 and per_segment(a, c1).tolist() == [0, 64] * 8
        i = np.arange(G)
        assert all(np.unique(lay["by_wave"][(i // 64) % 4 == w]).size == 1 for w in range(4))
        assert all(np.unique(lay["by_segment_group"][i // 256 == g]).size == 1 for g in range(4))
        assert np.unique(lay["by_wave"]).size == 4 and np.unique(lay["by_segment_group"]).size == 4
        assert all(lay[name].size % G != 0 for name in lay if name.endswith("_then_tail"))


@pytest.mark.parametrize("fmt,name", CASES)
def test_cpu_statements_on_every_layout(oracle, fmt, name):
    cls = P.layout(P.CLASSES[fmt], name)
    x = P.BLOCKS_WITH_CLASSES[fmt](cls, 7)     # (the builder asserts the classes with the statement's own classifier)
    y = forward(fmt, oracle, x)
    assert np.array_equal(inverse(fmt, oracle, y), x)
    if fmt == "bc7":
        assert np.array_equal(y, onp.transform_bc7(x))
        assert np.array_equal(onp.untransform_bc7(y), x)
    check_by_hand(cls, records(fmt, oracle, x), y)


@pytest.mark.parametrize("fmt", FORMATS)
def test_cpu_statements_on_all_layouts_in_one_buffer(oracle, fmt):
    cls, x = P.all_layouts_then_tail(fmt, 777, 3)
    assert cls.size > 20 * G and cls.size % G == 777
    y = forward(fmt, oracle, x)
    assert np.array_equal(inverse(fmt, oracle, y), x)
    if fmt == "bc7":
        assert np.array_equal(y, onp.transform_bc7(x))
    check_by_hand(cls, records(fmt, oracle, x), y)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mods(pkg):
    from dxt_lossless_transform_amd import batch, bc6h, bc7

    return {"bc7": bc7, "bc6h": bc6h, "batch": batch}


def calls(mods, fmt):
    m = mods[fmt]
    return (getattr(m, f"transform_{fmt}"), getattr(m, f"untransform_{fmt}"), getattr(m, f"transform_{fmt}_range"),
            getattr(m, f"transform_{fmt}_sharded"))


def device_round_trip(mods, fmt, oracle, x, tag):
    """forward of x and inverse of the CPU statement's output through the device call, each into a buffer with 64 guard bytes
    on either side; returns the CPU statement's output"""
    import torch

    dev = torch.device("cuda:0")
    fwd, inv, _, _ = calls(mods, fmt)
    want = forward(fmt, oracle, x)
    nb = x.size
    dst = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    back = torch.full((nb + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    fwd(torch.from_numpy(x).to(dev), dst[GUARD:GUARD + nb])
    inv(torch.from_numpy(want).to(dev), back[GUARD:GUARD + nb])
    torch.cuda.synchronize()
    got, rt = dst.cpu().numpy(), back.cpu().numpy()
    assert np.array_equal(got[GUARD:GUARD + nb], want), ("forward",) + tag
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + nb:] == 0xA5).all(), ("forward wrote outside",) + tag
    assert np.array_equal(rt[GUARD:GUARD + nb], x), ("inverse",) + tag
    assert (rt[:GUARD] == 0x5A).all() and (rt[GUARD + nb:] == 0x5A).all(), ("inverse wrote outside",) + tag
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,name", CASES)
def test_gpu_every_layout(mods, oracle, fmt, name):
    device_round_trip(mods, fmt, oracle, P.blocks_of_layout(fmt, name, 11), (fmt, name))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_all_layouts_in_one_buffer_through_every_entry_point(mods, oracle, fmt):
    import torch

    dev = torch.device("cuda:0")
    fwd, inv, ranged, sharded = calls(mods, fmt)
    cls, x = P.all_layouts_then_tail(fmt, 777, 5)
    n = cls.size
    want = device_round_trip(mods, fmt, oracle, x, (fmt, "device"))
    # the range call, one granule per call and the tail part with the last one
    cuts = list(range(0, n - n % G, G)) + [n]
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(want).to(dev)
    soa = torch.full((16 * n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    back = torch.full((16 * n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    for a, b in zip(cuts, cuts[1:]):
        ranged(False, xd[16 * a:16 * b], soa[GUARD:GUARD + 16 * n], n, a, b - a)
    for a, b in reversed(list(zip(cuts, cuts[1:]))):
        ranged(True, wd, back[GUARD + 16 * a:GUARD + 16 * b], n, a, b - a)
    torch.cuda.synchronize()
    got, rt = soa.cpu().numpy(), back.cpu().numpy()
    assert np.array_equal(got[GUARD:-GUARD], want) and (got[:GUARD] == 0xA5).all() and (got[-GUARD:] == 0xA5).all(), (fmt, "ranges")
    assert np.array_equal(rt[GUARD:-GUARD], x) and (rt[:GUARD] == 0x5A).all() and (rt[-GUARD:] == 0x5A).all(), (fmt, "ranges, inverse")
    # host pointers: the staged call and the sharded call
    for label, f, b in (("host", fwd, inv), ("sharded", lambda i, o: sharded(i, o, 3), lambda i, o: sharded(i, o, 3, inverse=True))):
        y = np.full(16 * n + GUARD, 0xA5, dtype=np.uint8)
        z = np.full(16 * n + GUARD, 0x5A, dtype=np.uint8)
        f(x, y[:16 * n])
        b(want, z[:16 * n])
        assert np.array_equal(y[:16 * n], want) and (y[16 * n:] == 0xA5).all(), (fmt, label)
        assert np.array_equal(z[:16 * n], x) and (z[16 * n:] == 0x5A).all(), (fmt, label, "inverse")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_every_tail_length_in_one_batch(mods, oracle, fmt):
    """1023 buffers of 1..1023 blocks in one batch call: the batch's tail-part kernel at every block count (dead lanes carry
    class 9 / 15), round-robin classes for odd counts and raw bytes for even ones; then the inverse batch over the CPU
    statement's outputs.  All buffers in one arena, 64 guard bytes behind each."""
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x7A11 + len(fmt))
    counts = list(range(1, G))
    xs = [P.tail_blocks(fmt, n, rng) for n in counts]
    wants = [forward(fmt, oracle, x) for x in xs]
    offs, at = [], GUARD
    for n in counts:
        offs.append(at)
        at += 16 * n + GUARD
    for inv, srcs, expect, fill in ((False, xs, wants, 0xA5), (True, wants, xs, 0x5A)):
        h = np.zeros(at, dtype=np.uint8)
        for o, s in zip(offs, srcs):
            h[o:o + s.size] = s
        src = torch.from_numpy(h).to(dev)
        dst = torch.full((at,), fill, dtype=torch.uint8, device=dev)
        mods["batch"].transform_batch([(fmt, inv, src[o:o + 16 * n], dst[o:o + 16 * n], None) for n, o in zip(counts, offs)])
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert (got[:GUARD] == fill).all()
        for n, o, e in zip(counts, offs, expect):
            assert np.array_equal(got[o:o + 16 * n], e), (fmt, "inverse" if inv else "forward", n)
            assert (got[o + 16 * n:o + 16 * n + GUARD] == fill).all(), (fmt, "inverse" if inv else "forward", n, "wrote outside")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_one_granule_plus_sampled_tail_lengths(mods, oracle, fmt):
    """1024 + t blocks through the single device call (a main-part launch and a tail-part launch) for 64 seeded values of t"""
    rng = np.random.default_rng(0x7A12 + len(fmt))
    for t in sorted(rng.choice(np.arange(1, G), size=64, replace=False).tolist()):
        x = np.concatenate([P.tail_blocks(fmt, G, rng), P.tail_blocks(fmt, t, rng)])
        device_round_trip(mods, fmt, oracle, x, (fmt, G + t))
