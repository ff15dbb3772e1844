"""The entropy estimator on the MI355X (csrc/entropy_kernels.hip, include/dxtlt_entropy_estimator.h) against its CPU statement
(tests/entropy_ref.py, docs/ESTIMATOR.md "The entropy estimator, version 1"): every number exact."""
import ctypes as C

import numpy as np
import pytest

import entropy_ref as R
import pixels_ref

pytestmark = pytest.mark.gpu

W = R.W
LENGTHS = [0, 1, 3, 4, 15, 16, 17, 255, 256, 257, W - 1, W, W + 1, 2 * W + 5, 3 * W]
RESIDUES = list(range(16)) + [31, 63, 64, 127]
KINDS = ["random", "constant", "two_values", "equal", "ramp"]
SLOT = 3 * W + 256        # the longest section behind the largest residue, rounded up


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def E(pkg):
    from dxt_lossless_transform_amd import estimator

    assert estimator.entropy_version() == R.VERSION
    return estimator


def section_data(kind, n, rng):
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "constant":                                   # every lane on one bin: the LDS worst case
        return np.full(n, 0xFF, dtype=np.uint8)
    if kind == "two_values":                                 # n - 1 / 1 in every window
        x = np.full(n, 0x40, dtype=np.uint8)
        x[W - 1::W] = 0x41
        if n % W:
            x[n - 1] = 0x41
        return x
    if kind == "equal":                                      # every value equally often (as far as n allows), shuffled
        return rng.permutation(np.arange(n, dtype=np.int64) & 0xFF).astype(np.uint8)
    return ((np.arange(n, dtype=np.int64) // 7) & 0xFF).astype(np.uint8)      # a ramp: runs of seven


@pytest.mark.parametrize("kind", KINDS)
def test_every_length_at_every_residue_in_one_call(E, dev, kind):
    """15 lengths x 20 base residues = 300 sections in ONE call (19 launches of 16 sections and the finishing launch), d_out
    between sentinel words."""
    import torch

    rng = np.random.default_rng(KINDS.index(kind) + 0xE270)
    cases = [(n, r) for n in LENGTHS for r in RESIDUES]
    arena = np.full(len(cases) * SLOT, 0xA5, dtype=np.uint8)
    want = []
    for k, (n, r) in enumerate(cases):
        x = section_data(kind, n, rng)
        arena[k * SLOT + r:k * SLOT + r + n] = x
        want.append(R.estimate(x))
    d = torch.from_numpy(arena).to(dev)                      # torch allocations are 256-byte aligned: slot bases are too
    assert d.data_ptr() % 256 == 0
    out = torch.full((len(cases) + 2,), -0x5E5E5E5E, dtype=torch.int64, device=dev)
    E.estimate_entropy_sizes([d[k * SLOT + r:k * SLOT + r + n] for k, (n, r) in enumerate(cases)], out[1:-1])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == got[-1] == -0x5E5E5E5E
    bad = [(cases[k], int(got[1 + k]), want[k]) for k in range(len(cases)) if got[1 + k] != want[k]]
    assert not bad, bad[:8]
    assert torch.equal(d.cpu(), torch.from_numpy(arena))     # sections are read only
    if kind == "constant":
        assert set(want) == {0}
    if kind == "equal":
        assert want[cases.index((W, 0))] == W


def test_forty_overlapping_sections(E, dev):
    """40 sections of one buffer, overlapping one another: three launches, each section's own number"""
    import torch

    rng = np.random.default_rng(40)
    x = np.concatenate([rng.integers(0, 8, 2 * W, dtype=np.uint8), rng.integers(0, 256, 2 * W + 100, dtype=np.uint8)])
    d = torch.from_numpy(x).to(dev)
    spans = [(37 * k, 37 * k + 1000 + 3001 * k) for k in range(40)]
    assert spans[-1][1] <= x.size and spans[1][0] < spans[0][1]
    out = torch.zeros(40, dtype=torch.int64, device=dev)
    E.estimate_entropy_sizes([d[a:b] for a, b in spans], out)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [R.estimate(x[a:b]) for a, b in spans]


def test_worked_vector_and_single_section_calls(E, dev):
    import torch

    v = np.frombuffer(R.WORKED_VECTOR, dtype=np.uint8).copy()
    assert E.estimate_entropy_size(torch.from_numpy(v).to(dev)) == R.WORKED_ESTIMATE
    rng = np.random.default_rng(5)
    x = rng.integers(0, 50, 5 * W + 321, dtype=np.uint8)
    d = torch.from_numpy(x).to(dev)
    for a, b in ((0, x.size), (1, x.size - 2), (W + 7, 4 * W + 7), (3, 3)):
        want = R.estimate(x[a:b])
        assert E.estimate_entropy_size(d[a:b]) == want                  # dxtlt_estimate_entropy_size_device
        assert E.estimate_entropy_size(x[a:b].copy()) == want           # dxtlt_estimate_entropy_size: host pointer
    # the vtable: what an estimator callback of an auto transform would call
    e = C.cast(E.builtin_entropy_estimator(), C.POINTER(pixels_ref.Estimator)).contents
    size = C.c_size_t(0)
    assert e.MaxCompressedSize(None, x.size, C.byref(size)) == 0 and size.value == 0
    assert e.EstimateCompressedSize(None, x.ctypes.data, x.size, None, 0, C.byref(size)) == 0
    assert size.value == R.estimate(x)


def test_capturable_and_replayed(E, dev):
    """dxtlt_estimate_entropy_sizes_device only enqueues: captured into a graph, replayed once, equal to the eager call; the
    waiting single-section call refuses the capturing stream."""
    import torch

    rng = np.random.default_rng(77)
    xs = [rng.integers(0, 1 + 13 * k, 1000 + 20000 * k, dtype=np.uint8) for k in range(1, 19)]      # two launches
    ds = [torch.from_numpy(x).to(dev) for x in xs]
    eager = torch.zeros(len(xs), dtype=torch.int64, device=dev)
    E.estimate_entropy_sizes(ds, eager)                                  # (also the warm-up outside the capture)
    torch.cuda.synchronize()
    assert eager.cpu().tolist() == [R.estimate(x) for x in xs]
    out = torch.zeros(len(xs), dtype=torch.int64, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        E.estimate_entropy_sizes(ds, out)
        one = C.c_uint64()
        rc = E._l().dxtlt_estimate_entropy_size_device(ds[0].data_ptr(), ds[0].numel(), torch.cuda.current_stream().cuda_stream,
                                                       C.byref(one))
    assert rc == 2
    assert int(out.abs().sum().item()) == 0                              # nothing ran during the capture
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
