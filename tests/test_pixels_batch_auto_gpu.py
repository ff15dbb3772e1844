"""dxtlt_transform_pixels_batch_auto_device on the MI355X (csrc/pixel_batch_auto_api.cpp; include/dxtlt_pixels.h) against its CPU
statement -- tests/pixels_ref.py for the bytes, tests/entropy_ref.py (R.auto) for the six totals and the pick -- and against
dxtlt_transform_pixels_auto_device on every item alone.  All outputs of a call lie in ONE arena between guard bytes."""
import ctypes as C
import threading

import numpy as np
import pytest

import entropy_ref as R
import pixels_auto_data as D
import pixels_batch_util as U

RESIDUES = [0, 1, 8, 15]


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return U.load(pkg)


_INPUTS = {}


def inputs():
    """[(name, B, flat bytes, input residue)]: slices of the r2-256 mip chain (the first candidate wins) and of random walks (the
    fourth) at every pixel count, a buffer of zeros (all six totals tie at 0: the first stays), a buffer of 0x7F (the last two tie at 0:
    the fifth stays) and an empty item, for both pixel sizes"""
    if not _INPUTS:
        chain = np.ascontiguousarray(D.data_sets()[2][1])
        assert chain.shape == (87381, 4)
        items = []
        for B in (4, 3):
            walks = D.random_walks(B, 87381, 11 + B)
            for k, P in enumerate(U.AUTO_COUNTS):
                items.append((f"chain {B} {P}", B, np.ascontiguousarray(chain[:P, :B]).reshape(-1), RESIDUES[k % 4]))
                items.append((f"walks {B} {P}", B, np.ascontiguousarray(walks[:P]).reshape(-1), RESIDUES[(k + 2) % 4]))
            items.append((f"constant {B}", B, np.zeros(B * 5000, dtype=np.uint8), RESIDUES[B % 4]))
            items.append((f"grey {B}", B, np.full(B * 5000, 0x7F, dtype=np.uint8), RESIDUES[(B + 1) % 4]))
            items.append((f"empty {B}", B, np.zeros(0, dtype=np.uint8), 0))
        _INPUTS["items"] = items
        _INPUTS["ref"] = [R.auto(flat, B) if flat.size else ([], 0, flat) for _n, B, flat, _r in items]
    return _INPUTS["items"], _INPUTS["ref"]


def test_the_reference_picks_of_the_inputs_have_three_outcomes():
    """no device: the first candidate alone at the top, the fourth, and a tie of all six that keeps the first"""
    items, ref = inputs()
    outcomes = set()
    for (name, _B, flat, _r), (totals, at, _out) in zip(items, ref):
        if flat.size:
            outcomes.add((at, len(set(totals)) == 1))
        if name.startswith("constant"):
            assert len(set(totals)) == 1 and at == 0
        if name.startswith("grey"):
            assert totals[4] == totals[5] == min(totals) < totals[0] and at == 4
    assert {(0, False), (3, False), (0, True), (4, False)} <= outcomes
    assert ref[[n for n, *_ in items].index("chain 4 87381")][1] == 0 and ref[[n for n, *_ in items].index("walks 4 87381")][1] == 3
    assert {r for *_x, r in items} == set(RESIDUES) and {B for _n, B, _f, _r in items} == {3, 4}


def auto_items(arenas, specs):
    arr = (U.AutoItem * len(specs))()
    for k, (_name, B, flat, _r) in enumerate(specs):
        arr[k].d_input, arr[k].d_output = (arenas.in_ptr(k), arenas.out_ptr(k)) if flat.size else (None, None)
        arr[k].len, arr[k].pixel_bytes, arr[k].decorrelate, arr[k].layout = flat.size, B, 0xEE, 0xEE
    return arr


def totals_of(lib, k):
    buf = (C.c_uint64 * 8)()
    n = lib.dxtlt_debug_pixels_batch_auto_last_totals(k, buf, 8)
    return [int(v) for v in buf[:n]]


def last_of(lib):
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    lib.dxtlt_debug_pixels_batch_auto_last(out)
    return list(out)


def estimation_of(lib):
    a, b = C.c_uint64(99), C.c_uint64(99)
    lib.dxtlt_debug_auto_last_estimation(C.byref(a), C.byref(b))
    return a.value, b.value


def run_auto(lib, dev, specs, ref, stream=None):
    """one call over `specs`; results, totals and bytes against the statement; returns (arenas, host arena, [(decorrelate, layout)])"""
    import torch

    arenas = U.Arenas(dev, [s[2] for s in specs], [s[3] for s in specs], [(3 * k + s[3]) % U.LINE for k, s in enumerate(specs)])
    arr = auto_items(arenas, specs)
    rc = lib.dxtlt_transform_pixels_batch_auto_device(arr, len(specs), stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.dxtlt_last_error()
    totals = [totals_of(lib, k) for k in range(len(specs))]
    host = arenas.check()
    choices = []
    for k, ((name, _B, flat, _r), (want_totals, at, want)) in enumerate(zip(specs, ref)):
        choices.append((bool(arr[k].decorrelate), int(arr[k].layout)))
        assert totals[k] == want_totals, name
        assert choices[k] == R.CANDIDATES[at], name
        assert np.array_equal(arenas.output(host, k), want), name
    return arenas, host, choices


@pytest.mark.gpu
def test_results_totals_and_bytes_equal_the_statement_and_the_single_call(lib, dev):
    import torch

    specs, ref = inputs()
    arenas, host, choices = run_auto(lib, dev, specs, ref)
    assert last_of(lib) == [1, 1, 2, 1] and estimation_of(lib) == (0, 0)
    # every item alone through the single call: the same choice, totals and bytes
    single = U.Arenas(dev, [s[2] for s in specs], [s[3] for s in specs], [(3 * k + s[3]) % U.LINE for k, s in enumerate(specs)])
    stream = torch.cuda.current_stream().cuda_stream
    for k, (name, B, flat, _r) in enumerate(specs):
        dec, lay = C.c_bool(), C.c_uint8(9)
        ptrs = (single.in_ptr(k), single.out_ptr(k)) if flat.size else (None, None)
        assert lib.dxtlt_transform_pixels_auto_device(*ptrs, flat.size, B, stream, C.byref(dec), C.byref(lay)) == 0, lib.dxtlt_last_error()
        buf = (C.c_uint64 * 8)()
        n = lib.dxtlt_debug_pixels_auto_last_totals(buf, 8)
        assert [int(v) for v in buf[:n]] == ref[k][0], name
        assert (dec.value, lay.value) == choices[k], name
    assert np.array_equal(single.check(), host)


@pytest.mark.gpu
def test_one_wait_and_the_same_launches_for_1_and_200_items(lib, dev):
    specs, ref = inputs()
    chain = specs[[s[0] for s in specs].index("chain 4 87381")][2]
    one = [("one", 4, chain[:4 * 4097], 8)]
    many = [(f"slice {k}", 4, chain[4 * 300 * k:4 * (300 * k + 200 + 19 * (k % 50))], RESIDUES[k % 4]) for k in range(200)]
    counts = []
    for batch in (one, many):
        run_auto(lib, dev, batch, [R.auto(s[2], 4) for s in batch])
        counts.append(last_of(lib))
        assert estimation_of(lib) == (0, 0)                       # no estimation bytes downloaded, no callback
    assert counts[0] == counts[1] == [1, 1, 1, 1]                 # waits, chunks, candidate launches, estimator launches


@pytest.mark.gpu
def test_chunks_give_the_same_totals_choices_and_bytes(lib, dev):
    specs, ref = inputs()
    by_name = {s[0]: k for k, s in enumerate(specs)}
    small = [by_name[f"{kind} {B} 4097"] for kind in ("chain", "walks") for B in (4, 3)]
    order = (small * 3) + [by_name["walks 4 87381"]]                  # 12 items of 16 388 or 12 291 bytes, then one of 349 524
    batch = [specs[k] for k in order]
    batch_ref = [ref[k] for k in order]
    _a, whole, whole_choices = run_auto(lib, dev, batch, batch_ref)
    assert last_of(lib) == [1, 1, 2, 1]
    # slices of 81 940 and 61 455 bytes, padded to 81 952 and 61 456: four items -- one of each kind -- are 286 816 bytes; the last item's is 1 747 620
    lib.dxtlt_debug_batch_auto_arena_cap(286_816)
    try:
        _a, cut, cut_choices = run_auto(lib, dev, batch, batch_ref)
        assert last_of(lib) == [1, 4, 3 * 2 + 1, 4]
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)
    assert cut_choices == whole_choices and np.array_equal(cut, whole)


def winners():
    """the twelve inputs of pixels_auto_data.winner_sets as specs, with their statement: every candidate the strict winner once per
    pixel size"""
    if "winners" not in _INPUTS:
        specs = [(name, B, px.reshape(-1), RESIDUES[k % 4]) for k, (name, B, px, _want) in enumerate(D.winner_sets())]
        _INPUTS["winners"] = (specs, [R.auto(flat, B) for _n, B, flat, _r in specs])
    return _INPUTS["winners"]


def test_the_reference_picks_every_candidate_strictly():
    """no device: the six reference picks per pixel size are exactly {0, 1, 2, 3, 4, 5}, each with its total below every other"""
    specs, ref = winners()
    for B in (4, 3):
        picks = []
        for (name, b, flat, _r), (totals, at, _out), (_n, _b, _px, want) in zip(specs, ref, D.winner_sets()):
            if b == B:
                assert flat.size == B * D.WINNER_PIXELS and at == want, name
                assert all(totals[at] < t for i, t in enumerate(totals) if i != at), (name, totals)
                picks.append(at)
        assert sorted(picks) == [0, 1, 2, 3, 4, 5], B


@pytest.mark.gpu
def test_every_candidate_wins_in_one_call_in_chunks_and_as_the_single_call(lib, dev):
    import torch

    specs, ref = winners()
    arenas, whole, whole_choices = run_auto(lib, dev, specs, ref)
    assert last_of(lib) == [1, 1, 2, 1]
    assert {R.CANDIDATES.index(c) for c in whole_choices[:6]} == {R.CANDIDATES.index(c) for c in whole_choices[6:]} == set(range(6))
    # slices of 327 680 and 245 760 bytes: five 4-byte items alone, the sixth with the first 3-byte item, then two, two and one
    lib.dxtlt_debug_batch_auto_arena_cap(600_000)
    try:
        _a, cut, cut_choices = run_auto(lib, dev, specs, ref)
        assert last_of(lib) == [1, 9, 10, 9]
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)
    assert cut_choices == whole_choices and np.array_equal(cut, whole)
    # every item alone through the single call: the same choice, totals and bytes
    single = U.Arenas(dev, [s[2] for s in specs], [s[3] for s in specs], [(3 * k + s[3]) % U.LINE for k, s in enumerate(specs)])
    stream = torch.cuda.current_stream().cuda_stream
    for k, (name, B, flat, _r) in enumerate(specs):
        dec, lay = C.c_bool(), C.c_uint8(9)
        rc = lib.dxtlt_transform_pixels_auto_device(single.in_ptr(k), single.out_ptr(k), flat.size, B, stream, C.byref(dec), C.byref(lay))
        assert rc == 0, lib.dxtlt_last_error()
        buf = (C.c_uint64 * 8)()
        n = lib.dxtlt_debug_pixels_auto_last_totals(buf, 8)
        assert [int(v) for v in buf[:n]] == ref[k][0], name
        assert (dec.value, lay.value) == whole_choices[k], name
    assert np.array_equal(single.check(), whole)


@pytest.mark.gpu
def test_refusals_enqueue_nothing_and_leave_the_results_alone(lib, dev):
    import torch

    specs, _ref = inputs()
    batch = [specs[0], specs[1], specs[2]]
    stream = torch.cuda.current_stream().cuda_stream
    # an output over the input of another item
    arenas = U.Arenas(dev, [s[2] for s in batch], [0, 1, 8], [0, 3, 5])
    arr = auto_items(arenas, batch)
    arr[2].d_output = arenas.in_ptr(0) + 1
    assert lib.dxtlt_transform_pixels_batch_auto_device(arr, 3, stream) == 2 and b"overlaps" in lib.dxtlt_last_error()
    assert [(a.decorrelate, a.layout) for a in arr] == [(0xEE, 0xEE)] * 3 and last_of(lib) == [0, 0, 0, 0]
    arenas.check(written=())
    # a capturing stream
    arr = auto_items(arenas, batch)
    x = torch.arange(400, dtype=torch.uint8, device=dev)
    y = torch.zeros_like(x)
    assert lib.dxtlt_transform_pixels_device(x.data_ptr(), y.data_ptr(), 400, 4, False, 0, stream) == 0      # module load outside the capture
    torch.cuda.synchronize()
    y.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        rc = lib.dxtlt_transform_pixels_batch_auto_device(arr, 3, s)
        error = lib.dxtlt_last_error()
        marker = lib.dxtlt_transform_pixels_device(x.data_ptr(), y.data_ptr(), 400, 4, False, 0, s)          # capturable
    assert rc == 2 and b"capturable" in error and marker == 0
    assert [(a.decorrelate, a.layout) for a in arr] == [(0xEE, 0xEE)] * 3 and last_of(lib) == [0, 0, 0, 0]
    graph.replay()                                                                                        # the capture is still alive
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    arenas.check(written=())


def on_a_fresh_thread(fn):
    """fn() on a thread of its own -- no table staging, counters or arena yet -- and its result or its exception here"""
    box = []

    def work():
        try:
            box.append((True, fn()))
        except BaseException as e:          # carried to the test's thread
            box.append((False, e))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    if not box[0][0]:
        raise box[0][1]
    return box[0][1]


@pytest.mark.gpu
def test_the_block_and_the_pixel_call_share_one_threads_buffers(lib, dev, oracle, pkg):
    """dxtlt_transform_batch_auto_device and this call stage their tables and read their counters back through the SAME per-thread
    buffers (csrc/batch_auto_common.h): block, pixel, block, pixel on one thread and one stream, every batch in three chunks or
    more, give what each batch gives alone on a fresh thread -- choices, totals, bytes and counts -- and what the CPU statements say."""
    import torch

    import batch_auto_util as BU
    import test_batch_auto_gpu as BG

    block_lib = BU.load(pkg)
    cap = 20_000
    # the 256-lane workgroup edges with two BC1 / BC4 blocks per lane, and an empty item per kind
    kinds = [("bc1", True), ("bc3", False), ("bc4", False), ("bc5", False)]
    block_specs = [(fmt, blocks, (i + j) % 4, 60 + i, use_all) for i, (fmt, use_all) in enumerate(kinds)
                   for j, blocks in enumerate((0, 1, 2, 3, 511, 512, 513))]
    blocks = BG.Batch(dev, block_specs, oracle)
    specs, ref = inputs()
    by_name = {s[0]: k for k, s in enumerate(specs)}
    # (the empty item in front: behind an item larger than the cap it would be a chunk without an estimator launch)
    first = [by_name["empty 4"]] + [by_name[f"chain {B} {P}"] for B in (4, 3) for P in U.AUTO_COUNTS[:3]]
    second = ([by_name["empty 3"]] + [by_name[f"{kind} {B} {P}"] for kind in ("chain", "walks") for B in (4, 3) for P in U.AUTO_COUNTS[:4]]) * 3
    # the second pixel batch outgrows the counters the block batch left behind (BatchAutoBuffers::reserve: half as many again and
    # 64), and with them its tables: 144 bytes of sections per item against 120 sections and 24 entries in all
    block_counters = sum(len(BU.shown_lengths(s[0], s[1] * BU.BLOCK[s[0]], s[4])) for s in block_specs)
    assert len(first) < len(second) and 6 * len(first) < block_counters and 6 * len(second) > block_counters + block_counters // 2 + 64

    def run_blocks(stream):
        blocks.reset()
        assert blocks.call(block_lib, stream.cuda_stream) == 0, block_lib.dxtlt_last_error()
        torch.cuda.synchronize()
        got = blocks.check_against_cpu(block_lib)
        counts = BG.last(block_lib)
        assert counts[0] == 1 and counts[1] >= 3 and counts[3] == counts[1], counts
        return [(c, o.tobytes(), t) for c, o, t in got], counts

    def run_pixels(which, stream):
        batch = [specs[k] for k in which]
        _a, host, choices = run_auto(lib, dev, batch, [ref[k] for k in which], stream.cuda_stream)
        counts = last_of(lib)
        assert counts[0] == 1 and counts[1] >= 3 and counts[3] == counts[1] and estimation_of(lib) == (0, 0), counts
        return host.tobytes(), choices, [totals_of(lib, k) for k in range(len(batch))], counts

    def on_one_thread(*runs):
        def work():
            torch.cuda.set_device(dev)
            stream = torch.cuda.Stream(device=dev)
            lib.dxtlt_debug_batch_auto_arena_cap(cap)            # per thread, for both calls
            with torch.cuda.stream(stream):
                return [run(stream) for run in runs]
        return on_a_fresh_thread(work)

    pixels_first, pixels_second = (lambda s: run_pixels(first, s)), (lambda s: run_pixels(second, s))
    alone = [on_one_thread(run)[0] for run in (run_blocks, pixels_first, pixels_second)]
    together = on_one_thread(run_blocks, pixels_first, run_blocks, pixels_second)
    assert together == [alone[0], alone[1], alone[0], alone[2]]


@pytest.mark.gpu
def test_two_threads_with_their_own_streams(lib, dev):
    import torch

    specs, ref = inputs()
    halves = [(specs[0::2], ref[0::2]), (specs[1::2], ref[1::2])]
    errors = []

    def work(half):
        try:
            torch.cuda.set_device(dev)
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for _ in range(2):
                    run_auto(lib, dev, half[0], half[1], stream.cuda_stream)
        except BaseException as e:          # carried to the test's thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(h,)) for h in halves]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
