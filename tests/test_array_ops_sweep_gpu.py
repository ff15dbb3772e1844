"""The stand-alone array operations swept on the device, byte for byte against the oracle: the colour-array kernels of
csrc/color565_ops.hip (ycocg, recorrelate-split, split-endpoints) and decode_blocks / count_pixel_differences of
csrc/bcn_decode.hip, with the second iteration of the two host slice loops of csrc/decode_api.cpp.

The case lists are tests/array_ops_cases.py; tests/test_array_ops_cases.py proves without a device which route, lane counts and
grid each case takes.  Every test that runs many launches puts them into arenas (tests/pixels_gpu_common.py): every output between
256 bytes of 0xA5, all launches issued through the C ABI `_device` calls on the current stream, one synchronise, one download, one
comparison with the expected image; every guard byte and every source byte is unchanged.  Expected bytes are computed once per
(operation, variant, count) and do not depend on a residue.  Every address a call receives lies inside an arena of the test."""
import ctypes as C

import numpy as np
import pytest

import array_ops_cases as K
from pixels_gpu_common import FILL, OK, Arena, check_image, device_arena
from test_color565 import oracle_table

pytestmark = pytest.mark.gpu
per_format = pytest.mark.parametrize("fmt", K.FORMATS)
per_direction = pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
SOURCE_FILL = 0x3C


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    d = torch.device("cuda:0")
    torch.zeros(1, dtype=torch.uint8, device=d)
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def lib(pkg):
    from dxt_lossless_transform_amd import color565, decode

    color565._l()
    return K.declare(decode._l())


@pytest.fixture(scope="module")
def tables(oracle):
    """[(variant, inverse)] -> the oracle's image of every colour; variant 0 is the identity"""
    t = {(v, inv): oracle_table(oracle, v, inv) for v in (1, 2, 3) for inv in (False, True)}
    t[(0, False)] = t[(0, True)] = np.arange(65536, dtype="<u2")
    return t


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Run:
    """Launches of one test: sources in `sources` arenas (one range per key and residue), outputs in one arena between guards"""

    def __init__(self, sources=1):
        self.src, self.src_at = [Arena() for _ in range(sources)], [{} for _ in range(sources)]
        self.out, self.placed, self.preset, self.calls = Arena(), [], [], []

    def source(self, key, data, residue, which=0):
        """offset of `data` at `residue` in source arena `which`; `key` names the array"""
        at = self.src_at[which]
        if (key, residue) not in at:
            at[(key, residue)] = (self.src[which].place(residue, data.size), data)
        return at[(key, residue)][0]

    def output(self, residue, want, tag, preset=None):
        """offset of an output that must hold `want` afterwards; `preset`: what it holds before (an in-place call's input)"""
        off = self.out.place(residue, want.size)
        self.placed.append((off, want, tag))
        if preset is not None:
            assert preset.size == want.size
            self.preset.append((off, preset))
        return off

    def call(self, fn, tag):
        """fn(source arena addresses, output arena address, stream) -> status"""
        self.calls.append((fn, tag))

    def go(self, dev):
        import torch

        h_src = []
        for arena, at in zip(self.src, self.src_at):
            h = np.full(arena.size(), SOURCE_FILL, dtype=np.uint8)
            for off, data in at.values():
                h[off:off + data.size] = data
            h_src.append(h)
        h_out = np.full(self.out.size(), FILL, dtype=np.uint8)
        for off, data in self.preset:
            h_out[off:off + data.size] = data
        d_src, d_out = [device_arena(dev, h) for h in h_src], device_arena(dev, h_out)
        S, O = [d.data_ptr() for d in d_src], d_out.data_ptr()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for fn, tag in self.calls:
                rc = fn(S, O, stream)
                assert rc == OK, (rc, tag)
            torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        check_image(got, self.placed, "output")
        for d, h in zip(d_src, h_src):
            assert np.array_equal(d.cpu().numpy(), h), "a call changed a source arena"


# ---- a. ycocg ------------------------------------------------------------------------------------------------------------------------
_COLOURS = np.random.default_rng(0xC565).integers(0, 65536, 4200 + 64, dtype=np.uint16).astype("<u2")
_YCOCG_IO = {}


def ycocg_io(tables, variant, inverse, n):
    """(input bytes, expected bytes) of n colours: forward colours -> the oracle's table; inverse that image -> back to the colours"""
    key = (variant, inverse, n)
    if key not in _YCOCG_IO:
        x = _COLOURS[n % 64:n % 64 + n]
        y = tables[(variant, False)][x]
        _YCOCG_IO[key] = (as_bytes(y), as_bytes(x)) if inverse else (as_bytes(x), as_bytes(y))
    return _YCOCG_IO[key]


def ycocg_function(lib, inverse):
    return lib.dxtlt_color565_recorrelate_ycocg_r_device if inverse else lib.dxtlt_color565_decorrelate_ycocg_r_device


def run_ycocg(lib, dev, tables, variant, inverse, cases):
    f, run = ycocg_function(lib, inverse), Run()
    for n, s, d in cases:
        src, want = ycocg_io(tables, variant, inverse, n)
        tag = ("ycocg", variant, "inverse" if inverse else "forward", n, s, d)
        if d is None:                                                        # in place: the output starts as the input
            o = run.output(s, want, tag, preset=src)
            run.call(lambda S, O, st, o=o, n=n: f(O + o, O + o, n, variant, st), tag)
        else:
            a, o = run.source(n, src, s), run.output(d, want, tag)
            run.call(lambda S, O, st, a=a, o=o, n=n: f(S[0] + a, O + o, n, variant, st), tag)
    run.go(dev)


@per_direction
@pytest.mark.parametrize("variant", K.YCOCG_VARIANTS)
def test_ycocg_every_offset_pair(lib, dev, tables, variant, inverse):
    """2051 colours at all 256 (source, destination) residues mod 16 and in place at all 16"""
    run_ycocg(lib, dev, tables, variant, inverse, K.ycocg_offset_cases())


@per_direction
@pytest.mark.parametrize("variant", K.YCOCG_VARIANTS)
def test_ycocg_every_count(lib, dev, tables, variant, inverse):
    """639 counts on the vector route: every number of singles, behind whole workgroups and across a workgroup boundary"""
    run_ycocg(lib, dev, tables, variant, inverse, K.ycocg_count_cases())


# ---- b. the two colours of a dword -----------------------------------------------------------------------------------------------------
def lane_pairs():
    """(524 288, 2) colour pairs (lo, hi), 2 MiB: for every colour c, c in the low half against 0x0000, 0xFFFF, its complement
    and a fixed permutation of it in the high half; then the same four partners in the low half against c in the high half"""
    c = np.arange(65536, dtype=np.int64)
    partners = [np.zeros_like(c), np.full_like(c, 0xFFFF), c ^ 0xFFFF, (c * 40503 + 12345) & 0xFFFF]
    assert sorted(partners[3].tolist()) == c.tolist()
    lo_fixed = np.concatenate([np.stack([c, p], axis=1) for p in partners])
    hi_fixed = np.concatenate([np.stack([p, c], axis=1) for p in partners])
    return np.concatenate([lo_fixed, hi_fixed]).astype("<u2")


@per_direction
@pytest.mark.parametrize("variant", K.YCOCG_VARIANTS)
def test_ycocg_pair_lanes_are_independent(lib, dev, tables, variant, inverse):
    """Every output colour is the table entry of its own input colour, whatever shares its dword: on the vector route; 2 bytes
    off, where every colour is alone in its register; 4 bytes off."""
    pairs = lane_pairs()
    assert pairs.shape == (8 * 65536, 2) and pairs.nbytes == 2 << 20
    for half in (0, 1):                                                      # every colour in either half, each against the extremes
        for other in (0x0000, 0xFFFF):
            assert len(np.unique(pairs[pairs[:, 1 - half] == other][:, half])) == 65536
    colours = pairs.reshape(-1)
    src, want = as_bytes(colours), as_bytes(tables[(variant, inverse)][colours])
    f, run = ycocg_function(lib, inverse), Run()
    for residue in (0, 2, 4):
        tag = ("pair lanes", variant, inverse, residue)
        a, o = run.source("pairs", src, residue), run.output(residue, want, tag)
        run.call(lambda S, O, st, a=a, o=o: f(S[0] + a, O + o, colours.size, variant, st), tag)
    assert bool(K.ycocg_plan(lib, (colours.size, 0, 0)).vector) and not K.ycocg_plan(lib, (colours.size, 2, 2)).vector
    run.go(dev)


# ---- c. recorrelate split, split endpoints ------------------------------------------------------------------------------------------------
_C0 = np.random.default_rng(0x5C0).integers(0, 65536, 2100 + 64, dtype=np.uint16).astype("<u2")
_C1 = np.random.default_rng(0x5C1).integers(0, 65536, 2100 + 64, dtype=np.uint16).astype("<u2")
_SPLIT_IO = {}


def split_io(tables, variant, pairs):
    """(src0 bytes, src1 bytes, expected bytes): dst[2k] = recorrelate(src0[k]), dst[2k + 1] = recorrelate(src1[k])"""
    key = (variant, pairs)
    if key not in _SPLIT_IO:
        c0, c1 = _C0[pairs % 64:pairs % 64 + pairs], _C1[pairs % 64:pairs % 64 + pairs]
        want = tables[(variant, True)][np.stack([c0, c1], axis=1).reshape(-1)]
        _SPLIT_IO[key] = (as_bytes(c0), as_bytes(c1), as_bytes(want))
    return _SPLIT_IO[key]


def run_split(lib, dev, tables, variant, cases):
    f, run = lib.dxtlt_color565_recorrelate_ycocg_r_split_device, Run(sources=2)
    for pairs, s0, s1, d in cases:
        b0, b1, want = split_io(tables, variant, pairs)
        tag = ("recorrelate split", variant, pairs, s0, s1, d)
        a0, a1, o = run.source(pairs, b0, s0, 0), run.source(pairs, b1, s1, 1), run.output(d, want, tag)
        run.call(lambda S, O, st, a0=a0, a1=a1, o=o, n=2 * pairs: f(S[0] + a0, S[1] + a1, O + o, n, variant, st), tag)
    run.go(dev)


@pytest.mark.parametrize("variant", K.SPLIT_VARIANTS)
def test_recorrelate_split_every_offset_triple(lib, dev, tables, variant):
    """1027 pairs from three separate buffers: both sources at every residue mod 16, the destination at eight"""
    run_split(lib, dev, tables, variant, K.split_offset_cases())


@pytest.mark.parametrize("variant", K.SPLIT_VARIANTS)
def test_recorrelate_split_every_count(lib, dev, tables, variant):
    """323 pair counts on the vector route of device pointers: 0, 1, 2 and 3 single pairs behind the vector lanes"""
    run_split(lib, dev, tables, variant, K.split_count_cases())


_ENDPOINT_BYTES = np.random.default_rng(0xE9D).integers(0, 256, 4 * (2100 + 64), dtype=np.uint8)
_ENDPOINT_IO = {}


def endpoint_io(oracle, pairs):
    if pairs not in _ENDPOINT_IO:
        x = _ENDPOINT_BYTES[4 * (pairs % 64):4 * (pairs % 64 + pairs)]
        _ENDPOINT_IO[pairs] = (x, oracle.split_565_color_endpoints(x))
    return _ENDPOINT_IO[pairs]


def run_endpoints(lib, dev, oracle, cases):
    """the expected bytes are both halves, all c0 then all c1; the byte behind the second half is a guard byte"""
    f, run = lib.dxtlt_split_565_color_endpoints_device, Run()
    for pairs, i, o_res in cases:
        src, want = endpoint_io(oracle, pairs)
        tag = ("split endpoints", pairs, i, o_res)
        a, o = run.source(pairs, src, i), run.output(o_res, want, tag)
        run.call(lambda S, O, st, a=a, o=o, n=4 * pairs: f(S[0] + a, O + o, n, st), tag)
    run.go(dev)


def test_split_endpoints_every_offset_pair(lib, dev, oracle):
    run_endpoints(lib, dev, oracle, K.endpoint_offset_cases())


def test_split_endpoints_every_count(lib, dev, oracle):
    run_endpoints(lib, dev, oracle, K.endpoint_count_cases())


# ---- d. decode ----------------------------------------------------------------------------------------------------------------------------
_POOL = {}


def pool(oracle, fmt):
    """(pool bytes, the oracle's pixels of the pool)"""
    if fmt not in _POOL:
        blocks = K.block_pool(fmt).reshape(-1)
        px = oracle.decode_blocks(fmt, blocks)
        px.setflags(write=False)
        _POOL[fmt] = (blocks, px)
    return _POOL[fmt]


def run_decode(lib, dev, oracle, fmt, cases):
    f, run, bs = getattr(lib, f"dxtlt_decode_{fmt}_blocks_device"), Run(), K.BLOCK[fmt]
    blocks, px = pool(oracle, fmt)
    for n, i, o_res in cases:
        w = K.pool_window(n)
        tag = ("decode", fmt, n, i, o_res)
        a, o = run.source(n, blocks[bs * w:bs * (w + n)], i), run.output(o_res, px[64 * w:64 * (w + n)], tag)
        run.call(lambda S, O, st, a=a, o=o, n=n: f(S[0] + a, bs * n, O + o, 64 * n, st), tag)
    run.go(dev)


@per_format
def test_decode_every_offset_pair(lib, dev, oracle, fmt):
    """259 blocks at every (input, output) offset 0..16"""
    run_decode(lib, dev, oracle, fmt, K.decode_offset_cases())


@per_format
def test_decode_every_count(lib, dev, oracle, fmt):
    run_decode(lib, dev, oracle, fmt, K.decode_count_cases())


# ---- e. the difference count at every length -----------------------------------------------------------------------------------------------
def pixel_flags(oracle, fmt, a, b):
    n = a.shape[0]
    pa, pb = (oracle.decode_blocks(fmt, x.reshape(-1)).reshape(n, 64) for x in (a, b))
    return (pa != pb).any(axis=1)


@per_format
def test_difference_every_prefix_length(lib, dev, oracle, fmt):
    """count(a[:m], b[:m]) for every m in 1..1061, each into its own 8-byte slot: every n % 512 residue, the last block differing
    and not, the lanes past the end reading a last block that differs; vector loads and byte loads"""
    bs, n = K.BLOCK[fmt], K.DIFF_BLOCKS
    a, b = K.difference_pair(fmt, n, 0xD1F0 + K.KIND[fmt])
    flags = pixel_flags(oracle, fmt, a, b)
    kinds = K.block_kinds(n)
    assert np.array_equal(flags, kinds == K.DIFFERENT) and np.array_equal((a != b).any(axis=1), kinds != K.EQUAL)
    assert all((kinds == k).any() for k in (K.EQUAL, K.EQUIVALENT, K.DIFFERENT))
    assert flags[0] and flags[3] and not flags[1]        # the prefix of 4 begins and ends with a block that differs; that of 2 does not end so
    want = as_bytes(np.cumsum(flags).astype("<u8"))
    f, run = lib.dxtlt_count_pixel_differences_device, Run(sources=2)
    for ra, rb in K.DIFF_POINTERS:
        pa, pb = run.source("a", a.reshape(-1), ra, 0), run.source("b", b.reshape(-1), rb, 1)
        o = run.output(0, want, ("difference", fmt, ra, rb))
        for m in K.difference_prefix_lengths():
            run.call(lambda S, O, st, pa=pa, pb=pb, slot=o + 8 * (m - 1), m=m: f(K.KIND[fmt], S[0] + pa, S[1] + pb, bs * m, O + slot, st),
                     ("difference", fmt, ra, rb, m))
    run.go(dev)


# ---- f. the difference count across the grid -----------------------------------------------------------------------------------------------
@per_format
def test_difference_walks_the_grid(lib, dev, oracle, fmt):
    """2 * 2^21 + 512 + 37 blocks: every workgroup of the capped grid takes two steps, the first two a third.  A 1021-block
    pattern pair tiled on the device; the expected count is whole periods of the oracle's flags plus the rest."""
    import torch

    bs, n, period = K.BLOCK[fmt], K.WALK_BLOCKS, K.POOL_BLOCKS
    pa, pb = K.difference_pair(fmt, period, 0xD1F1 + K.KIND[fmt])
    flags = pixel_flags(oracle, fmt, pa, pb)
    assert 0 < int(flags.sum()) < period
    expected = n // period * int(flags.sum()) + int(flags[:n % period].sum())
    sa, sb = K.solid_pair(fmt, period)
    assert pixel_flags(oracle, fmt, sa, sb).all()

    def tiled(pattern, off=0):
        """n blocks of the tiled pattern, `off` bytes behind a 256-byte aligned address"""
        t = torch.from_numpy(pattern.reshape(-1).copy()).to(dev).repeat(n // period + 1)
        buf = torch.full((n * bs + 512,), SOURCE_FILL, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 256 == 0
        buf[off:off + n * bs] = t[:n * bs]
        return buf

    a, a1, b, s, t = tiled(pa), tiled(pa, 1), tiled(pb), tiled(sa), tiled(sb)
    A, A1, B, S_, T = a.data_ptr(), a1.data_ptr() + 1, b.data_ptr(), s.data_ptr(), t.data_ptr()
    launches = [("aligned", A, B, expected), ("a one byte off", A1, B, expected), ("a against itself", A, A, 0),
                ("arguments swapped", B, A, expected), ("swapped, one byte off", B, A1, expected), ("every block differs", S_, T, n)]
    want = as_bytes(np.array([w for _, _, _, w in launches], dtype="<u8"))
    run = Run(sources=0)
    o = run.output(0, want, ("walk", fmt, [name for name, _, _, _ in launches]))
    for k, (name, x, y, _) in enumerate(launches):
        run.call(lambda S, O, st, x=x, y=y, k=k: lib.dxtlt_count_pixel_differences_device(K.KIND[fmt], x, y, n * bs, O + o + 8 * k, st),
                 ("walk", fmt, name))
    for first, vector in ((A, True), (A1, False)):
        p = K.difference_plan(lib, fmt, n, first, B)
        assert (p.workgroups, p.steps, bool(p.vector)) == (K.DIFF_GRID, 3, vector)
    run.go(dev)
    for buf, pattern, off in ((a, pa, 0), (a1, pa, 1), (b, pb, 0)):          # the sources are unchanged: head, last period, fill behind
        head = buf[:off + period * bs].cpu().numpy()
        assert (head[:off] == SOURCE_FILL).all() and np.array_equal(head[off:], pattern.reshape(-1))
        assert (buf[off + n * bs:].cpu().numpy() == SOURCE_FILL).all()


# ---- g. the host calls past one slice --------------------------------------------------------------------------------------------------------
def host_decode_crosses_a_slice(lib, oracle, fmt):
    """one slice + 259 blocks through dxtlt_decode_bcN_blocks: the second slice reads and writes behind the first"""
    bs, period = K.BLOCK[fmt], K.POOL_BLOCKS
    n = K.slices(lib)[0] + 259
    blocks, px = pool(oracle, fmt)
    whole, rest = divmod(n, period)
    assert whole >= 2 and 0 < rest
    x = np.concatenate([np.tile(blocks, whole), blocks[:bs * rest]])
    out = np.full(64 * n + 256, FILL, dtype=np.uint8)
    rc = getattr(lib, f"dxtlt_decode_{fmt}_blocks")(x.ctypes.data, x.size, out.ctypes.data, 64 * n)
    assert rc == OK
    assert (out[64 * n:] == FILL).all()
    periods = out[:64 * period * whole].reshape(whole, 64 * period)
    bad = np.flatnonzero((periods != px[None, :]).any(axis=1))
    assert bad.size == 0, (fmt, "first wrong period", int(bad[0]), "of", whole, "first wrong block",
                           int(bad[0]) * period + int(np.flatnonzero(periods[bad[0]] != px)[0]) // 64)
    wrong = np.flatnonzero(out[64 * period * whole:64 * n] != px[:64 * rest])
    assert wrong.size == 0, (fmt, "first wrong block", period * whole + int(wrong[0]) // 64, "of", n)


def host_difference_crosses_a_slice(lib, oracle, fmt):
    """one slice + 549 blocks per array through dxtlt_count_pixel_differences: the counts of both slices are added"""
    bs, period = K.BLOCK[fmt], K.POOL_BLOCKS
    first = K.slices(lib)[1] // bs                       # blocks of slice 0
    n = first + 549
    pa, pb = K.difference_pair(fmt, period, 0xD1F1 + K.KIND[fmt])
    flags = pixel_flags(oracle, fmt, pa, pb)
    sa, sb = K.solid_pair(fmt, 1)
    assert pixel_flags(oracle, fmt, sa, sb).all()
    whole, rest = divmod(n, period)
    a = np.concatenate([np.tile(pa.reshape(-1), whole), pa.reshape(-1)[:bs * rest]])
    b = np.concatenate([np.tile(pb.reshape(-1), whole), pb.reshape(-1)[:bs * rest]])
    forced = (first - 1, first, n - 1)                   # the last block of slice 0, the first of slice 1, the last of all
    for at in forced:
        a[bs * at:bs * (at + 1)], b[bs * at:bs * (at + 1)] = sa[0], sb[0]
    # whole periods and the rest of the pattern, then the three forced blocks: each counts once, and where the pattern's own block
    # at that place already differed it must not count twice
    expected = whole * int(flags.sum()) + int(flags[:rest].sum()) + sum(1 - int(flags[at % period]) for at in forced)
    count = C.c_uint64(1 << 63)
    assert lib.dxtlt_count_pixel_differences(K.KIND[fmt], a.ctypes.data, b.ctypes.data, a.size, C.byref(count)) == OK
    assert count.value == expected, (fmt, count.value, expected)
    assert lib.dxtlt_count_pixel_differences(K.KIND[fmt], b.ctypes.data, a.ctypes.data, a.size, C.byref(count)) == OK
    assert count.value == expected


@pytest.mark.parametrize("fmt", ["bc1", "bc3"])
@pytest.mark.parametrize("call", ["decode", "difference"])
def test_host_calls_cross_a_slice(lib, dev, oracle, call, fmt):
    """The slice sizes come from dxtlt_debug_array_op_slices; one case per call and format, so that none takes long"""
    (host_decode_crosses_a_slice if call == "decode" else host_difference_crosses_a_slice)(lib, oracle, fmt)
