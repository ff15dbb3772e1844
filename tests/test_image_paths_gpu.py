"""Every store and lookup path of the image decode sinks on the MI355X, under byte comparison with the CPU decoders.

The calls are the lists of tests/test_image_paths_layout.py (build_cases), whose no-device test proves which cells of
(tile kind x wave path x lane path x store class x clip class) they reach; here they run through
dxtlt_untransform_decode_image_device / dxtlt_decode_image_device and their channel twins, dxtlt_untransform_decode_images_device /
dxtlt_decode_images_device and dxtlt_untransform_decode_images_batch_device.  The input is the CPU statement's transform
(oracle.transform, bc45_ref.transform), the expected pixels the oracle's decoder rearranged into rows (image_regions_common).

As in tests/test_alignment_sweep.py the outputs of a whole list sit side by side in ONE 0xA5-filled device arena, every one at the
pixel-pointer residue (modulo 256) its case asks for with 256 guard bytes or more around it; the sources sit in a second arena.
All calls are enqueued, then one synchronisation and one download: the image rows, the pitch padding, the bytes behind every last
row and the guards are one comparison with the arena's expected bytes, and the sources must be unchanged.  A failure names the case
and the census cell (tests/image_paths.py) of the block that owns the first wrong byte."""
import bisect
import ctypes as C

import numpy as np
import pytest

import image_paths
from image_batch_common import batch_items, load
from image_regions_common import BLOCK, FMT_ID, FMTS, OK, expected_buffer, image_of, reference, region_array
from test_image_paths_layout import build_cases, census_of

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


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
    l = load(pkg)
    vp, i32, u32, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
    for f in (l.dxtlt_decode_image_device, l.dxtlt_decode_channel_image_device):
        f.argtypes, f.restype = [i32, vp, u32, u32, vp, u64, vp], i32
    return l


def up256(x):
    return (x + 255) & ~255


class Arena:
    """byte ranges at chosen residues modulo 256 inside one buffer, GUARD or more bytes between neighbours and at both ends"""

    def __init__(self):
        self.at = 0

    def place(self, residue, nbytes):
        off = up256(self.at + GUARD) + residue
        self.at = off + nbytes
        return off

    def size(self):
        return up256(self.at + GUARD) + 256


def source_of(oracle, case):
    """(key, bytes) of the buffer a case reads: the transformed buffer, or for the plain decoders the blocks"""
    plain = case.entry.startswith("plain")
    x, t = reference(oracle, case.fmt, case.total, case.settings, case.seed)
    return (plain, case.fmt, case.total, None if plain else case.settings, case.seed, case.in_off), x if plain else t


class Staged:
    """the two arenas of a list of cases on the device: src_ptr[i] the source pointer of case i, out_ptr[i][k] the pixel pointer
    of its region k (0 for an empty region)"""

    def __init__(self, dev, oracle, cases):
        import torch

        self.cases = cases
        src, out = Arena(), Arena()
        placed, self.slots, src_off, out_off = {}, [], [], []
        for i, case in enumerate(cases):
            key, data = source_of(oracle, case)
            if key not in placed:
                placed[key] = (src.place(case.in_off, data.size), data)
            src_off.append(placed[key][0])
            offs = []
            for k, (_, w, h) in enumerate(case.regions):
                if w == 0 or h == 0:
                    offs.append(None)
                    continue
                offs.append(out.place(case.out_offs[k], case.pitches[k] * h))
                self.slots.append((offs[-1], case.pitches[k] * h, i, k))
            out_off.append(offs)
        self.h_src = np.full(src.size(), FILL, dtype=np.uint8)
        for off, data in placed.values():
            self.h_src[off:off + data.size] = data
        self.d_src = torch.from_numpy(self.h_src).to(dev)
        self.d_out = torch.full((out.size(),), FILL, dtype=torch.uint8, device=dev)
        assert self.d_src.data_ptr() % 256 == 0 and self.d_out.data_ptr() % 256 == 0, "the residues are taken from 256-byte aligned allocations"
        self.src_ptr = [self.d_src.data_ptr() + off for off in src_off]
        self.out_ptr = [[0 if off is None else self.d_out.data_ptr() + off for off in offs] for offs in out_off]
        for case, s, ptrs in zip(cases, self.src_ptr, self.out_ptr):
            assert s % 256 == case.in_off and all(p == 0 or p % 256 == o for p, o in zip(ptrs, case.out_offs))

    def check(self, lib, oracle, label):
        """after ONE synchronisation: every byte of the output arena and of the source arena"""
        got = self.d_out.cpu().numpy()
        want = np.full(got.size, FILL, dtype=np.uint8)
        for off, nbytes, i, k in self.slots:
            case = self.cases[i]
            want[off:off + nbytes] = expected_buffer(image_of(oracle, case.fmt, case.total, case.regions[k], case.seed), case.pitches[k])
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            at = int(bad[0])
            j = max(0, bisect.bisect_right([s[0] for s in self.slots], at) - 1)
            off, nbytes, i, k = self.slots[j]
            case = self.cases[i]
            if off <= at < off + nbytes:
                where = image_paths.cell_of_byte(case, census_of(lib, case), k, at - off)
                pytest.fail(f"{label}: {bad.size} wrong bytes, the first is byte {at - off} of region {k} {case.regions[k]} of [{case.name}] "
                            f"(got {got[at]:#x}, want {want[at]:#x}): {where}")
            if at < off:
                pytest.fail(f"{label}: {bad.size} wrong bytes, the first a guard byte {off - at} bytes in front of the first slot, region {k} "
                            f"{case.regions[k]} of [{case.name}]")
            pytest.fail(f"{label}: {bad.size} wrong bytes, the first a guard byte {at - off - nbytes} bytes behind region {k} "
                        f"{case.regions[k]} of [{case.name}]")
        assert np.array_equal(self.d_src.cpu().numpy(), self.h_src), (label, "a source buffer changed")


def stream_of(dev):
    import torch

    return torch.cuda.current_stream(dev).cuda_stream


def enqueue(lib, dev, case, src, outs):
    """one call of a single-image or regions case"""
    fmt, s, stream = case.fmt, case.settings, stream_of(dev)
    channel = fmt in ("bc4", "bc5")
    if case.entry in ("single", "plain single"):
        ((first, w, h),) = case.regions
        if case.entry == "plain single":
            f = lib.dxtlt_decode_channel_image_device if channel else lib.dxtlt_decode_image_device
            rc = f(FMT_ID[fmt], src + first * BLOCK[fmt], w, h, outs[0], case.pitches[0], stream)
        elif channel:
            rc = lib.dxtlt_untransform_decode_channel_image_device(FMT_ID[fmt], src, case.total, first, w, h, s[1], outs[0], case.pitches[0], stream)
        else:
            rc = lib.dxtlt_untransform_decode_image_device(FMT_ID[fmt], src, case.total, first, w, h, s[0], s[1], s[2], outs[0],
                                                           case.pitches[0], stream)
    else:
        arr = region_array(case.regions, [p or None for p in outs], case.pitches)
        if case.entry == "plain regions":
            rc = lib.dxtlt_decode_images_device(FMT_ID[fmt], src, case.total, arr, len(case.regions), stream)
        else:
            rc = lib.dxtlt_untransform_decode_images_device(FMT_ID[fmt], src, case.total, arr, len(case.regions), s[0], s[1], s[2], stream)
    assert rc == OK, (case.name, lib.dxtlt_last_error())


def run_calls(lib, dev, oracle, cases, label):
    import torch

    staged = Staged(dev, oracle, cases)
    for case, src, outs in zip(cases, staged.src_ptr, staged.out_ptr):
        enqueue(lib, dev, case, src, outs)
    torch.cuda.synchronize()
    staged.check(lib, oracle, label)


def enqueue_batch(lib, dev, staged, lo, hi, keep):
    """ONE batch call whose items are cases [lo, hi) of the staged list"""
    items = [image_paths.as_item(c) for c in staged.cases[lo:hi]]
    arr = batch_items(items, staged.src_ptr[lo:hi], [[p or None for p in ptrs] for ptrs in staged.out_ptr[lo:hi]], keep)
    keep.append(arr)
    assert lib.dxtlt_untransform_decode_images_batch_device(arr, len(items), stream_of(dev)) == OK, lib.dxtlt_last_error()


@pytest.mark.parametrize("fmt", FMTS)
def test_single_image_calls(lib, dev, oracle, fmt):
    """(a) and (b): the fused and the plain single-image decoders"""
    cases = build_cases(lib)
    run_calls(lib, dev, oracle, cases["single"][fmt] + cases["plain single"][fmt], f"single image {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
def test_region_calls(lib, dev, oracle, fmt):
    """(c): the fused and the plain regions call"""
    cases = build_cases(lib)
    run_calls(lib, dev, oracle, cases["regions"][fmt] + cases["plain regions"][fmt], f"regions {fmt}")


BATCH_CALLS = 6


def mixed(lists):
    """the formats' lists dealt into one, format after format"""
    out = []
    for i in range(max(len(l) for l in lists)):
        out += [l[i] for l in lists if i < len(l)]
    return out


def test_batch_calls(lib, dev, oracle):
    """(c) through the batch call: the tables of all five formats, mixed, in a few calls"""
    import torch

    cases = mixed([build_cases(lib)["batch"][fmt] for fmt in FMTS])
    staged = Staged(dev, oracle, cases)
    keep = []
    step = -(-len(cases) // BATCH_CALLS)
    for lo in range(0, len(cases), step):
        enqueue_batch(lib, dev, staged, lo, min(lo + step, len(cases)), keep)
    torch.cuda.synchronize()
    staged.check(lib, oracle, "batch")


@pytest.mark.parametrize("fmt", FMTS)
def test_random_region_tables(lib, dev, oracle, fmt):
    """(d): the seeded random tables through the fused and the plain regions call"""
    fused = build_cases(lib)["random regions"][fmt]
    plain = [c._replace(entry="plain regions", name=c.name.replace(" regions ", " plain regions ")) for c in fused]
    run_calls(lib, dev, oracle, fused + plain, f"random regions {fmt}")


def test_random_tables_in_batch_calls(lib, dev, oracle):
    import torch

    cases = mixed([build_cases(lib)["random batch"][fmt] for fmt in FMTS])
    staged = Staged(dev, oracle, cases)
    keep = []
    for lo in range(0, len(cases), 40):
        enqueue_batch(lib, dev, staged, lo, min(lo + 40, len(cases)), keep)
    torch.cuda.synchronize()
    staged.check(lib, oracle, "random batch")


def test_the_table_ring_three_times_round(lib, pkg, dev, oracle):
    """csrc/table_ring.h, which the image batch call shares with dxtlt_transform_batch_device: twelve image batch calls from one
    thread on torch's current stream without a synchronisation in between -- three times round the four slots, the tables growing
    from call to call so that slots are reallocated while earlier calls may still be in flight -- with six
    dxtlt_transform_batch_device calls on a second stream in between.  One synchronisation; every output of every call exact,
    every source unchanged."""
    import torch

    from dxt_lossless_transform_amd import batch

    pool = mixed([build_cases(lib)["random batch"][fmt] for fmt in FMTS])
    calls, cases = [], []
    for j in range(12):     # call j: 3 + 5 j items from a window that moves through the pool, its own outputs
        chosen = [pool[(11 * j + i) % len(pool)] for i in range(3 + 5 * j)]
        calls.append((len(cases), len(cases) + len(chosen)))
        cases += [c._replace(name=f"{c.name} in ring call {j}") for c in chosen]
    staged = Staged(dev, oracle, cases)
    # the transform calls: forward, the item count growing too
    plan = [("bc1", pkg.Bc1TransformSettings()), ("bc3", pkg.Bc3TransformSettings()), ("bc2", pkg.Bc2TransformSettings())]
    transforms = []
    for j in range(6):
        items, wants = [], []
        for i in range(2 + 3 * j):
            fmt, st = plan[(i + j) % 3]
            blocks = 300 + 97 * i + 1031 * j
            host = oracle.fill_splitmix64(blocks * pkg.BLOCK_BYTES[fmt], 0x7AB1E000 + 64 * j + i)
            x = torch.from_numpy(host).to(dev)
            y = torch.full_like(x, FILL)
            items.append((fmt, False, x, y, st))
            wants.append((host, oracle.transform(fmt, host, int(st.decorrelation_mode), st.split_colour_endpoints,
                                                 getattr(st, "split_alpha_endpoints", True))))
        transforms.append((items, wants))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    keep = []
    for j, (lo, hi) in enumerate(calls):
        enqueue_batch(lib, dev, staged, lo, hi, keep)
        if j % 2 == 1:
            with torch.cuda.stream(side):
                batch.transform_batch(transforms[j // 2][0])
    torch.cuda.synchronize()
    staged.check(lib, oracle, "table ring")
    for j, (items, wants) in enumerate(transforms):
        for (fmt, _, x, y, _), (host, want) in zip(items, wants):
            assert np.array_equal(y.cpu().numpy(), want), ("transform call", j, fmt, "differs from the CPU statement")
            assert np.array_equal(x.cpu().numpy(), host), ("transform call", j, fmt, "its input changed")
