"""dxtlt_transform_batch_auto_device on the MI355X (include/dxtlt_estimator.h, csrc/batch_auto_api.cpp, batch_auto_kernels.hip and
the table-driven launch of estimate_kernels.hip): for every item of a batch the choice, the totals compared and the output bytes
are those of the CPU statement (oracle/oracle_auto.py and tests/bc45_ref.py over tests/estimator_ref.py) -- never the library's
own single-buffer answer, except where a test says it compares the two -- with one stream wait per call."""
import ctypes as C

import numpy as np
import pytest

import batch_auto_util as U
import bc45_ref
import estimator_ref as R

pytestmark = pytest.mark.gpu

KINDS = [(f, u) for f in ("bc1", "bc2", "bc3") for u in (False, True)] + [("bc4", False), ("bc5", False)]
COUNTS = (0, 1, 2, 3, 129, 4097, 8191, 8192, 8193, 20_001)
FILL = 0xA5
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return U.load(pkg)


_cpu_cache = {}


def cpu_auto(spec, oracle):
    """spec = (fmt, blocks, style, seed, use_all) -> (input, choice (mode, split_alpha, split_colour), output, totals in candidate
    order); computed once per spec and shared"""
    if spec in _cpu_cache:
        return _cpu_cache[spec]
    fmt, blocks, style, seed, use_all = spec
    x = U.auto_input(fmt, blocks, style, seed)
    sizes = []

    def estimate(b):
        sizes.append(R.estimate(b))
        return sizes[-1]

    if fmt in ("bc4", "bc5"):
        split = bool(bc45_ref.auto_choice(fmt, x, estimate))
        choice, out, per = (0, int(split), 0), bc45_ref.transform(fmt, x, split), (1 if fmt == "bc4" else 2)
    else:
        from oracle import oracle_auto

        c, out, _ = oracle_auto.transform_auto(fmt, x, estimate, use_all)
        choice, out, per = tuple(int(v) for v in c), np.asarray(out), (2 if fmt == "bc3" else 1)
    totals = [sum(sizes[i:i + per]) for i in range(0, len(sizes), per)]
    x.setflags(write=False)
    _cpu_cache[spec] = (x, choice, out, totals)
    return _cpu_cache[spec]


def require_two_choices_per_format(specs, oracle):
    """the condition every test states on the CPU side: its items do not all favour the same settings"""
    seen = {}
    for s in specs:
        seen.setdefault(s[0], set()).add(cpu_auto(s, oracle)[1])
    assert all(len(v) >= 2 for v in seen.values()), seen


class Batch:
    """The items of `specs` side by side in one input pool and one output pool (16-byte aligned slots, GUARD fill bytes and
    more between them), item k's input `in_off[k]` and output `out_off[k]` bytes behind its slot's boundary."""

    def __init__(self, dev, specs, oracle, in_off=None, out_off=None):
        import torch

        self.specs, self.cpu = specs, [cpu_auto(s, oracle) for s in specs]
        n = len(specs)
        self.in_off, self.out_off = in_off or [0] * n, out_off or [0] * n
        self.at, at = [], 0
        for (x, *_), a, b in zip(self.cpu, self.in_off, self.out_off):
            at += GUARD + 16
            self.at.append(at)
            at = (at + max(a, b) + x.size + GUARD + 15) & ~15
        self.total = at + GUARD
        host = np.full(self.total, 0x3C, dtype=np.uint8)
        for (x, *_), at, a in zip(self.cpu, self.at, self.in_off):
            host[at + a:at + a + x.size] = x
        self.host_in = host
        self.d_in = torch.from_numpy(host).to(dev)
        self.d_out = torch.full((self.total,), FILL, dtype=torch.uint8, device=dev)
        assert self.d_in.data_ptr() % 16 == 0 and self.d_out.data_ptr() % 16 == 0
        self.items = U.make_items([(s[0], self.d_in.data_ptr() + at + a, self.d_out.data_ptr() + at + b, x.size, s[4])
                                   for s, (x, *_), at, a, b in zip(specs, self.cpu, self.at, self.in_off, self.out_off)])

    def reset(self):
        self.d_out.fill_(FILL)
        for it in self.items:
            it.decorrelation_mode = it.split_alpha_endpoints = it.split_colour_endpoints = 0xEE

    def call(self, lib, stream=None):
        import torch

        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        return lib.dxtlt_transform_batch_auto_device(self.items, len(self.specs), stream)

    def results(self, lib):
        """after the call and a device synchronise: per item (choice, bytes, totals); checks the inputs and every byte of the output
        pool outside the outputs (the 64 guard bytes on both sides of each among them)"""
        whole = self.d_out.cpu().numpy()
        assert np.array_equal(self.d_in.cpu().numpy(), self.host_in), "an input changed"
        outside = np.ones(self.total, dtype=bool)
        got = []
        buf = (C.c_uint64 * 16)()
        for k, ((x, *_), at, b, it) in enumerate(zip(self.cpu, self.at, self.out_off, self.items)):
            outside[at + b:at + b + x.size] = False
            n = lib.dxtlt_debug_batch_auto_last_totals(k, buf, 16)
            got.append(((it.decorrelation_mode, it.split_alpha_endpoints, it.split_colour_endpoints),
                        whole[at + b:at + b + x.size].copy(), [int(v) for v in buf[:n]]))
        assert (whole[outside] == FILL).all(), "wrote outside the outputs"
        return got

    def check_against_cpu(self, lib, got=None):
        got = self.results(lib) if got is None else got
        assert len(got) == len(self.specs)
        for k, (spec, (x, choice, out, totals), (g_choice, g_out, g_totals)) in enumerate(zip(self.specs, self.cpu, got)):
            assert g_choice == choice, (k, spec, g_choice, choice)
            assert g_totals == (totals if x.size else []), (k, spec)
            assert np.array_equal(g_out, out), (k, spec)
        return got

    def untouched(self):
        return bool((self.d_out == FILL).all().item()) and all(it.decorrelation_mode == 0xEE for it in self.items)


def last(lib):
    out = (C.c_uint64 * 4)()
    lib.dxtlt_debug_batch_auto_last(out)
    a, b = C.c_uint64(7), C.c_uint64(7)
    lib.dxtlt_debug_auto_last_estimation(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    return tuple(int(v) for v in out)


def planned_candidate_launches(lib, batch):
    """per chunk, what the planner (dxtlt_debug_plan_batch_auto, under the cap now set) says the call launches, each held to the
    distinct (format, use_all) pairs among the chunk's non-empty items"""
    n = len(batch.specs)
    items, chunks, count = (U.PlanItem * n)(), (U.PlanChunk * 4096)(), C.c_size_t()
    assert lib.dxtlt_debug_plan_batch_auto(batch.items, n, items, chunks, 4096, C.byref(count)) == 0
    per_chunk = []
    for ch in chunks[:count.value]:
        mine = batch.specs[ch.first_item:ch.first_item + ch.item_count]
        pairs = {(s[0], s[4]) for s in mine if s[1]}
        assert ch.candidate_launches == len(pairs)
        per_chunk.append(ch.candidate_launches)
    return per_chunk


def mixed_specs():
    return [(fmt, blocks, (i + j) % 4, 1 + i, use_all) for i, (fmt, use_all) in enumerate(KINDS) for j, blocks in enumerate(COUNTS)]


@pytest.fixture(scope="module")
def mixed(dev, oracle):
    specs = mixed_specs()
    require_two_choices_per_format(specs, oracle)
    return Batch(dev, specs, oracle)


def test_one_mixed_batch_against_the_cpu_statement(lib, mixed):
    import torch

    mixed.reset()
    assert mixed.call(lib) == 0, lib.dxtlt_last_error()
    torch.cuda.synchronize()
    mixed.check_against_cpu(lib)
    waits, chunks, candidate_launches, estimator_launches = last(lib)
    assert waits == 1 and chunks == 1
    assert candidate_launches == sum(planned_candidate_launches(lib, mixed)) == len(KINDS)
    assert estimator_launches == chunks


def test_input_and_output_pointers_off_alignment(lib, dev, oracle):
    import torch

    specs, in_off, out_off = [], [], []
    for i, (fmt, use_all) in enumerate(KINDS):
        for j, blocks in enumerate((3, 255, 4097)):
            for k, off in enumerate((1, 4, 8, 15)):
                specs.append((fmt, blocks, (i + j + k) % 4, 20 + k, use_all))
                in_off.append(off)
                out_off.append((1, 7, 3, 13)[(j + k) % 4])
    require_two_choices_per_format(specs, oracle)
    b = Batch(dev, specs, oracle, in_off, out_off)
    assert all(it.d_input % 16 == o and it.d_output % 2 == 1 for it, o in zip(b.items, in_off))
    assert b.call(lib) == 0, lib.dxtlt_last_error()
    torch.cuda.synchronize()
    b.check_against_cpu(lib)
    waits, chunks, candidate_launches, estimator_launches = last(lib)
    assert (waits, chunks, estimator_launches) == (1, 1, 1) and candidate_launches <= len(KINDS)


def test_many_tiny_items_twice(lib, dev, oracle):
    import torch

    specs = [("bc3" if k % 3 == 0 else "bc1", 1 + (k * 7) % 40, k % 4, k % 5, k % 2 == 1) for k in range(300)]
    # (four candidate tables of at most 100 entries so far.)  300 more of ONE kind, in between: a candidate table of about 400
    # entries, bisected past 64 and 256, beside the estimator's table of thousands
    specs = [s for k in range(300) for s in (specs[k], ("bc1", 1 + (k * 11) % 40, (k // 3) % 4, 5 + k % 3, False))]
    assert sum(1 for s in specs if s[0] == "bc1" and not s[4]) > 256
    require_two_choices_per_format(specs, oracle)
    b = Batch(dev, specs, oracle)
    runs = []
    for _ in range(2):
        b.reset()
        assert b.call(lib) == 0, lib.dxtlt_last_error()
        torch.cuda.synchronize()
        runs.append(b.check_against_cpu(lib))
        assert last(lib)[0] == 1 and last(lib)[2] <= 4
    for a, c in zip(*runs):
        assert a[0] == c[0] and a[2] == c[2] and np.array_equal(a[1], c[1])


def test_several_chunks_give_what_one_chunk_gives(lib, mixed):
    import torch

    mixed.reset()
    assert mixed.call(lib) == 0
    torch.cuda.synchronize()
    whole = mixed.results(lib)
    cap = 700_000                      # 20 001 BC3 blocks with all modes need 720 036 bytes: larger than the cap
    mixed.reset()
    lib.dxtlt_debug_batch_auto_arena_cap(cap)
    try:
        rc = mixed.call(lib)
        torch.cuda.synchronize()
        waits, chunks, candidate_launches, estimator_launches = last(lib)
        planned = planned_candidate_launches(lib, mixed)
    finally:
        lib.dxtlt_debug_batch_auto_arena_cap(0)
    assert rc == 0, lib.dxtlt_last_error()
    assert any(x.size // U.BLOCK[s[0]] * 36 > cap for s, (x, *_) in zip(mixed.specs, mixed.cpu) if s[0] == "bc3" and s[4])
    assert waits == 1 and chunks >= 3 and estimator_launches == chunks == len(planned)
    assert candidate_launches == sum(planned)          # per chunk: the distinct (format, use_all) pairs in it, no more
    got = mixed.check_against_cpu(lib)
    for a, c in zip(whole, got):
        assert a[0] == c[0] and a[2] == c[2] and np.array_equal(a[1], c[1])


def test_agreement_with_the_single_buffer_calls(lib, dev, mixed, pkg):
    import torch

    from dxt_lossless_transform_amd import estimator

    mixed.reset()
    assert mixed.call(lib) == 0
    torch.cuda.synchronize()
    got = mixed.results(lib)
    picked = [k for k, s in enumerate(mixed.specs) if s[1] in (3, 4097, 8193)][:16]
    assert len(picked) >= 12
    for k in picked:
        fmt, _blocks, _style, _seed, use_all = mixed.specs[k]
        x = torch.from_numpy(np.array(mixed.cpu[k][0])).to(dev)
        y = torch.zeros_like(x)
        s = estimator.transform_auto(fmt, x, y, use_all)
        torch.cuda.synchronize()
        single = (int(getattr(s, "decorrelation_mode", 0)), int(getattr(s, "split_alpha_endpoints", getattr(s, "split_endpoints", 0))),
                  int(getattr(s, "split_colour_endpoints", 0)))
        assert single == got[k][0], (k, mixed.specs[k])
        assert np.array_equal(y.cpu().numpy(), got[k][1]), (k, mixed.specs[k])
        assert estimator.last_auto_totals() == got[k][2], (k, mixed.specs[k])


def test_refusals_leave_every_output_untouched(lib, dev, oracle, pkg):
    import torch

    from dxt_lossless_transform_amd import estimator

    specs = [("bc1", 129, 0, 1, False), ("bc3", 255, 1, 2, True), ("bc5", 40, 2, 3, False)]
    b = Batch(dev, specs, oracle)
    assert lib.dxtlt_transform_batch_auto_device(None, 0, None) == 0
    # a capturing stream: an error at once, nothing enqueued, and the capture is still alive afterwards
    counters = torch.zeros(1, dtype=torch.int64, device=dev)
    estimator.estimate_sizes([b.d_in], counters)
    assert b.call(lib) == 0                                            # warm-up outside capture (module load)
    torch.cuda.synchronize()
    want = int(counters.item())
    counters.zero_()
    b.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = b.call(lib, torch.cuda.current_stream().cuda_stream)
        estimator.estimate_sizes([b.d_in], counters)                   # enqueue-only: capturable
    assert rc == 2 and b"capturable" in lib.dxtlt_last_error()
    assert last(lib) == (0, 0, 0, 0)
    torch.cuda.synchronize()
    assert b.untouched()
    graph.replay()
    torch.cuda.synchronize()
    assert int(counters.item()) == want and b.untouched()

    def refused(change, status):
        saved = [(it.d_input, it.d_output, it.len, it.format) for it in b.items]
        change(b.items)
        try:
            assert b.call(lib) == status, lib.dxtlt_last_error()
            torch.cuda.synchronize()
            assert b.untouched() and last(lib) == (0, 0, 0, 0)
        finally:
            for it, (i, o, n, f) in zip(b.items, saved):
                it.d_input, it.d_output, it.len, it.format = i, o, n, f

    def setter(k, **kw):
        def change(items):
            for name, v in kw.items():
                setattr(items[k], name, v)
        return change

    refused(setter(1, d_input=None), 2)
    refused(setter(2, d_output=None), 2)
    for f in (0, 6, 7):
        refused(setter(0, format=f), 2)
    refused(setter(1, len=255 * 16 - 8), 1)
    refused(setter(0, len=129 * 8 + 4), 1)
    refused(setter(2, d_output=b.items[1].d_output + 16), 2)          # two overlapping outputs
    refused(setter(2, d_output=b.items[0].d_input + 8), 2)            # an output over another item's input
    # and the batch still runs
    assert b.call(lib) == 0
    torch.cuda.synchronize()
    b.check_against_cpu(lib)


def test_two_calls_of_one_thread_on_two_streams_and_the_python_wrapper(lib, dev, oracle, pkg):
    import torch

    from dxt_lossless_transform_amd import batch, estimator

    halves = [[(fmt, blocks, (i + j + h) % 4, 30 + h, use_all) for i, (fmt, use_all) in enumerate(KINDS)
               for j, blocks in enumerate((255, 1023, 4097, 20_001))] for h in (0, 1)]     # every style per format
    for specs in halves:
        require_two_choices_per_format(specs, oracle)
    batches = [Batch(dev, specs, oracle) for specs in halves]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for _ in range(2):
        for b in batches:
            b.reset()
        torch.cuda.synchronize()
        # back to back: the second call fills the arena and the counters while the first call's transforms may still run
        totals = []
        for b, s in zip(batches, streams):
            assert b.call(lib, s.cuda_stream) == 0, lib.dxtlt_last_error()
            buf = (C.c_uint64 * 16)()
            totals.append([[int(v) for v in buf[:lib.dxtlt_debug_batch_auto_last_totals(k, buf, 16)]] for k in range(len(b.specs))])
        torch.cuda.synchronize()
        for b, t in zip(batches, totals):
            got = b.results(lib)
            b.check_against_cpu(lib, [(g[0], g[1], tk) for g, tk in zip(got, t)])

    # the Python wrapper on torch's current stream
    b = batches[0]
    outs = [torch.full((x.size,), FILL, dtype=torch.uint8, device=dev) for x, *_ in b.cpu]
    ins = [torch.from_numpy(np.array(x)).to(dev) for x, *_ in b.cpu]
    items = [(s[0], i, o, s[4]) for s, i, o in zip(b.specs, ins, outs)]
    with torch.cuda.stream(streams[1]):
        chosen = batch.transform_batch_auto(items)
        assert estimator.last_batch_auto()[0] == 1
    torch.cuda.synchronize()
    assert batch.transform_batch_auto([]) == [] and len(chosen) == len(items)
    for k, (s, (x, choice, out, _t), c, o) in enumerate(zip(b.specs, b.cpu, chosen, outs)):
        got = (int(getattr(c, "decorrelation_mode", 0)), int(getattr(c, "split_alpha_endpoints", getattr(c, "split_endpoints", 0))),
               int(getattr(c, "split_colour_endpoints", 0)))
        assert type(c).__name__ == f"Bc{s[0][2]}TransformSettings" and got == choice, (k, s)
        assert np.array_equal(o.cpu().numpy(), out), (k, s)


# ---------------------------------------------------------------------------------------------------------------
# The lane edges of the candidate kernels' one lane body (csrc/auto_candidate_lanes.h): the half lane of an odd BC1 / BC4 count
# alone (1), as lane 255 of workgroup 0 (511) and as lane 0 of workgroup 1 (513), none (512); the last lane of a workgroup and the
# first of the next for the formats of one block per lane.  Every case at 0, 4 and 1 bytes off a 16-byte boundary: the batched
# kernel's vector, dword and byte loads; the single-buffer call takes its candidate kernels at 0 and one transform per candidate else.
# ---------------------------------------------------------------------------------------------------------------
EDGE_COUNTS = {"bc1": (1, 2, 3, 511, 512, 513), "bc4": (1, 2, 3, 511, 512, 513),
               "bc2": (1, 255, 256, 257), "bc3": (1, 255, 256, 257), "bc5": (1, 255, 256, 257)}
EDGE_OFFSETS = (0, 4, 1)


def edge_cases():
    """(spec, input offset) per (kind, count, offset); the styles and seeds were chosen on the CPU so that edge_batch's condition holds"""
    return [((fmt, blocks, (i + j + k) % 4, 40 + k, use_all), off) for i, (fmt, use_all) in enumerate(KINDS)
            for j, blocks in enumerate(EDGE_COUNTS[fmt]) for k, off in enumerate(EDGE_OFFSETS)]


@pytest.fixture(scope="module")
def edge_batch(dev, oracle):
    cases = edge_cases()
    assert len(cases) == sum(len(EDGE_COUNTS[f]) for f, _ in KINDS) * len(EDGE_OFFSETS)       # no case is left out
    # stated on the CPU before the first device call: within every format and search depth the CPU statement makes at least two
    # different choices -- a single block ties by construction and counts towards neither
    seen = {}
    for s, _ in cases:
        if s[1] > 1:
            seen.setdefault((s[0], s[4]), set()).add(cpu_auto(s, oracle)[1])
    assert len(seen) == len(KINDS) and all(len(v) >= 2 for v in seen.values()), seen
    return Batch(dev, [s for s, _ in cases], oracle, [off for _, off in cases])


@pytest.fixture(scope="module")
def edge_runs(lib, dev, edge_batch, pkg):
    """ONE batched call over every case, then the single-buffer calls: the same inputs where they lie, into a pool of their own laid
    out like the batch's.  -> per case (batched, single), each (choice, bytes, totals); the bytes around every output are checked"""
    import torch

    from dxt_lossless_transform_amd import estimator

    b = edge_batch
    assert all(it.d_input % 16 == off for it, off in zip(b.items, b.in_off))
    b.reset()
    assert b.call(lib) == 0, lib.dxtlt_last_error()
    torch.cuda.synchronize()
    batched = b.results(lib)
    assert last(lib)[0] == 1
    pool = torch.full((b.total,), FILL, dtype=torch.uint8, device=dev)
    outside = np.ones(b.total, dtype=bool)
    chosen = []
    for spec, (x, *_), at, a in zip(b.specs, b.cpu, b.at, b.in_off):
        s = estimator.transform_auto(spec[0], b.d_in[at + a:at + a + x.size], pool[at:at + x.size], spec[4])
        chosen.append(((int(getattr(s, "decorrelation_mode", 0)), int(getattr(s, "split_alpha_endpoints", getattr(s, "split_endpoints", 0))),
                        int(getattr(s, "split_colour_endpoints", 0))), estimator.last_auto_totals()))
        outside[at:at + x.size] = False
    torch.cuda.synchronize()
    whole = pool.cpu().numpy()
    assert (whole[outside] == FILL).all(), "a single-buffer call wrote outside its output"
    return [(g, (c, whole[at:at + x.size], t)) for g, (c, t), (x, *_), at in zip(batched, chosen, b.cpu, b.at)]


@pytest.mark.parametrize("fmt,use_all", KINDS)
def test_lane_edges_batched_single_and_cpu_agree(edge_batch, edge_runs, fmt, use_all):
    mine = [k for k, s in enumerate(edge_batch.specs) if (s[0], s[4]) == (fmt, use_all)]
    assert len(mine) == len(EDGE_COUNTS[fmt]) * len(EDGE_OFFSETS)
    for k in mine:
        spec, (_x, choice, out, totals) = edge_batch.specs[k], edge_batch.cpu[k]
        for route, (g_choice, g_out, g_totals) in zip(("batched", "single"), edge_runs[k]):
            assert g_choice == choice, (route, spec, edge_batch.in_off[k], g_choice, choice)
            assert g_totals == totals, (route, spec, edge_batch.in_off[k])
            assert np.array_equal(g_out, out), (route, spec, edge_batch.in_off[k])
