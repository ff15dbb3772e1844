"""dxtlt_transform_pixels_batch_device on the MI355X (csrc/pixel_batch_api.cpp, pixel_batch_kernels.hip; include/dxtlt_pixels.h)
against tests/pixels_ref.py and against one single-buffer call per item.  Every call keeps all its outputs in ONE arena, each
between 256 guard bytes, and the guards, the gaps and every input are compared afterwards.  The case lists are built in
tests/pixels_batch_util.py; tests/test_pixels_batch_plan.py counts what they reach."""
import numpy as np
import pytest

import pixels_batch_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return U.load(pkg)


def run_batch(lib, dev, cases, seed=1):
    """the cases as one call; every output against the statement.  Returns (arenas, output arena on the host, the byte pairs)"""
    import torch

    pairs = U.source_bytes(cases, seed)
    arenas = U.Arenas(dev, [p[0] for p in pairs], [c[5] for c in cases], [c[6] for c in cases])
    arr = U.make_items(cases, arenas)
    rc = lib.dxtlt_transform_pixels_batch_device(arr, len(cases), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.dxtlt_last_error()
    host = arenas.check()
    for k, (_src, want) in enumerate(pairs):
        assert np.array_equal(arenas.output(host, k), want), (k, cases[k])
    return arenas, host, pairs


def test_every_class_in_one_call(lib, dev):
    cases = U.cases_every_class()
    run_batch(lib, dev, cases)            # (the inverse items' expected bytes are the pixels their inputs were made from)


@pytest.mark.parametrize("which", ["wide index", "long entries", 1, 2, 64, 65])
def test_lookup_both_arms(lib, dev, which):
    cases = U.cases_wide_lookup() if which == "wide index" else U.cases_long_entries() if which == "long entries" else U.cases_count(which)
    run_batch(lib, dev, cases, seed=7)


@pytest.mark.parametrize("B", [4, 3])
@pytest.mark.parametrize("inverse", [0, 1])
def test_every_residue_of_a_line_on_both_sides(lib, dev, B, inverse):
    run_batch(lib, dev, U.cases_alignment(B, inverse), seed=B + inverse)


def test_the_batch_equals_one_single_call_per_item(lib, dev):
    import torch

    cases = U.cases_mix()
    arenas, host, pairs = run_batch(lib, dev, cases, seed=3)
    single = U.Arenas(dev, [p[0] for p in pairs], [c[5] for c in cases], [c[6] for c in cases])
    stream = torch.cuda.current_stream().cuda_stream
    for k, (P, B, inv, dec, lay, _ri, _ro) in enumerate(cases):
        f = lib.dxtlt_untransform_pixels_device if inv else lib.dxtlt_transform_pixels_device
        assert f(single.in_ptr(k), single.out_ptr(k), P * B, B, bool(dec), lay, stream) == 0, lib.dxtlt_last_error()
    assert np.array_equal(single.check(), host)          # the whole arenas, byte for byte


def test_empty_items_and_an_empty_batch(lib, dev):
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    assert lib.dxtlt_transform_pixels_batch_device(None, 0, stream) == 0
    cases = [(0, 4, 0, 1, 2, 0, 0), (4097, 4, 0, 1, 2, 3, 5), (0, 3, 1, 0, 0, 0, 0), (17, 3, 1, 1, 1, 9, 1), (0, 4, 0, 1, 2, 0, 0)]
    run_batch(lib, dev, cases)


def test_a_refused_batch_writes_nothing(lib, dev):
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    cases = [(4097, 4, 0, 1, 2, 1, 2), (8193, 3, 1, 0, 1, 5, 9), (100, 4, 0, 0, 0, 0, 0)]
    pairs = U.source_bytes(cases)
    for defect in ("layout", "length", "overlap", "capture"):
        arenas = U.Arenas(dev, [p[0] for p in pairs], [c[5] for c in cases], [c[6] for c in cases])      # outputs poisoned with 0xEE
        arr = U.make_items(cases, arenas)
        if defect == "layout":
            arr[2].layout = 3
        elif defect == "length":
            arr[2].len = 4 * 100 + 1
        elif defect == "overlap":
            arr[2].d_output = arenas.out_ptr(0) + 4 * 4097 - 1                                              # the last byte of item 0's output
        if defect == "capture":
            warm = U.Arenas(dev, [p[0] for p in pairs], [c[5] for c in cases], [c[6] for c in cases])
            assert lib.dxtlt_transform_pixels_batch_device(U.make_items(cases, warm), 3, stream) == 0      # module load outside the capture
            torch.cuda.synchronize()
            x = torch.arange(400, dtype=torch.uint8, device=dev)
            y = torch.zeros_like(x)
            assert lib.dxtlt_transform_pixels_device(x.data_ptr(), y.data_ptr(), 400, 4, False, 0, stream) == 0
            torch.cuda.synchronize()
            y.zero_()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                s = torch.cuda.current_stream().cuda_stream
                rc = lib.dxtlt_transform_pixels_batch_device(arr, 3, s)
                error = lib.dxtlt_last_error()
                marker = lib.dxtlt_transform_pixels_device(x.data_ptr(), y.data_ptr(), 400, 4, False, 0, s)     # capturable
            assert rc == 2 and b"capturable" in error and marker == 0
            graph.replay()                                                                                  # the capture is still alive
            torch.cuda.synchronize()
            assert torch.equal(x, y)
        else:
            assert lib.dxtlt_transform_pixels_batch_device(arr, 3, stream) == (1 if defect == "length" else 2), defect
        arenas.check(written=())                                                                            # guards, gaps, inputs and every output
