"""The table-driven launch of the entropy estimator on the MI355X (csrc/entropy_kernels.hip: launch_entropy_table, through
dxtlt_debug_estimate_entropy_table_device) against tests/entropy_ref.py and against dxtlt_estimate_entropy_sizes_device: any
number of sections in one launch, every base residue, 256 guard bytes around every section, two entries on one counter."""
import ctypes as C

import numpy as np
import pytest

import entropy_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256
LENGTHS = [1, 15, 16, 17, 32767, 32768, 32769, 65536 + 5]
SENTINEL = 0x5A5A5A5A5A5A5A5A


class Section(C.Structure):                   # DxtltEstimateSection
    _fields_ = [("d_ptr", C.c_void_p), ("len", C.c_uint64)]


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    vp, sz, u64p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)
    l.dxtlt_debug_estimate_entropy_table_device.argtypes = [C.POINTER(Section), sz, vp, vp]
    l.dxtlt_debug_estimate_entropy_table_device.restype = C.c_int32
    l.dxtlt_debug_estimate_entropy_table_counters_device.argtypes = [C.POINTER(Section), C.POINTER(C.c_uint32), sz, sz, vp, vp]
    l.dxtlt_debug_estimate_entropy_table_counters_device.restype = C.c_int32
    l.dxtlt_estimate_entropy_sizes_device.argtypes = [C.POINTER(Section), sz, vp, vp]
    l.dxtlt_estimate_entropy_sizes_device.restype = C.c_int32
    l.dxtlt_last_error.restype = C.c_char_p
    return l


def data_of(kind, n, rng):
    if kind == 0:
        return np.full(n, 0xA7, dtype=np.uint8)                                   # constant
    if kind == 1:
        return rng.choice(np.array([3, 250], dtype=np.uint8), n)                   # two values
    if kind == 2:
        return rng.integers(0, 256, n, dtype=np.uint8)                             # uniform
    return (128 + np.clip(np.cumsum(rng.integers(-2, 3, n)), -120, 120)).astype(np.uint8)   # a walk


def sections_of(count, seed):
    """`count` sections: lengths of LENGTHS in turn, base k at residue k mod 16, the four kinds of data in turn; (arena on the host,
    [(offset, length)])"""
    rng = np.random.default_rng(seed)
    at, spans, parts = 0, [], []
    for k in range(count):
        n = LENGTHS[(k + k // len(LENGTHS)) % len(LENGTHS)]
        at += GUARD
        at += (k % 16 - at) % 16
        spans.append((at, n))
        parts.append(data_of(k % 4, n, rng))
        at += n
    host = np.full(at + GUARD, 0x11, dtype=np.uint8)
    for (o, n), d in zip(spans, parts):
        host[o:o + n] = d
    return host, spans


_REF = {}


def reference(count, seed):
    if (count, seed) not in _REF:
        host, spans = sections_of(count, seed)
        _REF[count, seed] = (host, spans, [R.estimate(host[o:o + n]) for o, n in spans])
    return _REF[count, seed]


@pytest.mark.parametrize("count", [1, 16, 17, 200])
def test_table_launch_equals_the_statement_and_the_argument_launch(lib, dev, count):
    import torch

    host, spans, want = reference(count, 100 + count)
    if count >= 16:
        assert {o % 16 for o, _n in spans} == set(range(16)) and {n for _o, n in spans} == set(LENGTHS)
    arena = torch.from_numpy(host).to(dev)
    assert arena.data_ptr() % 16 == 0
    before = arena.clone()
    secs = (Section * count)(*[Section(arena.data_ptr() + o, n) for o, n in spans])
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for f in (lib.dxtlt_debug_estimate_entropy_table_device, lib.dxtlt_estimate_entropy_sizes_device):
        out = torch.full((count + 2,), SENTINEL, dtype=torch.int64, device=dev)
        assert f(secs, count, stream, out.data_ptr() + 8) == 0, lib.dxtlt_last_error()
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.uint64)
        assert got[0] == SENTINEL and got[-1] == SENTINEL, "counters outside the call's own written"
        outs.append([int(v) for v in got[1:-1]])
    assert outs[0] == want
    assert outs[1] == want
    assert torch.equal(arena, before)


def test_entries_that_share_a_counter_and_sections_without_bytes(lib, dev):
    import torch

    host, spans, want = reference(17, 117)
    arena = torch.from_numpy(host).to(dev)
    count = len(spans) + 2
    secs = (Section * count)(*([Section(arena.data_ptr() + o, n) for o, n in spans] + [Section(None, 100), Section(arena.data_ptr(), 0)]))
    # sections 0 and 9 (1 byte and 16 bytes), 6 and 7 (32769 and 65541 bytes) share counters; the two without bytes have one each
    counters = list(range(len(spans))) + [len(spans), len(spans) + 1]
    counters[9], counters[7] = 0, 6
    out = torch.full((count + 2,), SENTINEL, dtype=torch.int64, device=dev)
    rc = lib.dxtlt_debug_estimate_entropy_table_counters_device(secs, (C.c_uint32 * count)(*counters), count, count,
                                                                torch.cuda.current_stream().cuda_stream, out.data_ptr() + 8)
    assert rc == 0, lib.dxtlt_last_error()
    torch.cuda.synchronize()
    got = [int(v) for v in out.cpu().numpy().astype(np.uint64)]
    assert got[0] == SENTINEL and got[-1] == SENTINEL
    cost = [R.section_cost(host[o:o + n]) for o, n in spans]
    expect = list(want) + [0, 0]
    expect[0] = (cost[0] + cost[9] + (1 << R.SHIFT) - 1) >> R.SHIFT            # ONE sum of q, rounded once
    expect[6] = (cost[6] + cost[7] + (1 << R.SHIFT) - 1) >> R.SHIFT
    expect[9] = expect[7] = 0
    assert got[1:-1] == expect
    assert expect[6] != want[6] + want[7] or expect[0] != want[0] + want[9]     # rounding the sum is not summing the rounded
    bad = (C.c_uint32 * count)(*([count] * count))
    assert lib.dxtlt_debug_estimate_entropy_table_counters_device(secs, bad, count, count, None, out.data_ptr() + 8) == 2
