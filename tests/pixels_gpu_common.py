"""What the device tests of the pixel transform share (tests/test_pixels_gpu.py, tests/test_pixels_sweep_gpu.py) and what the
fuzz campaign draws from (tools/fuzz_gpu.py --pixels): a single guarded device buffer, an arena of many outputs between guard
bytes with one upload, one synchronise and one download per run, and the draw of a combination case."""
import bisect
import collections

import numpy as np

import pixels_ref as R

GUARD = 64
OK, E_ARGUMENT = 0, 2


class Guarded:
    """`n` device bytes at offset `off` from a 256-byte aligned address, GUARD + off bytes of 0xA5 in front and GUARD behind"""

    def __init__(self, dev, n, off=0, data=None):
        import torch

        self.n, self.at = n, GUARD + off
        self.base = torch.full((self.at + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        assert self.base.data_ptr() % 256 == 0
        if data is not None:
            self.base[self.at:self.at + n].copy_(torch.from_numpy(np.ascontiguousarray(data)).to(dev))
        self.ptr = self.base.data_ptr() + self.at

    def bytes(self):
        """the payload, after checking the guards"""
        host = self.base.cpu().numpy()
        assert (host[:self.at] == 0xA5).all() and (host[self.at + self.n:] == 0xA5).all(), "guard bytes were written"
        return host[self.at:self.at + self.n]


def device_call(lib, dev, inverse, data, B, decorrelate, layout, in_off=0, out_off=0):
    import torch

    src, dst = Guarded(dev, data.size, in_off, data), Guarded(dev, data.size, out_off)
    f = lib.dxtlt_untransform_pixels_device if inverse else lib.dxtlt_transform_pixels_device
    with torch.cuda.device(dev):
        rc = f(src.ptr, dst.ptr, data.size, B, decorrelate, layout, torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), data)
    return dst.bytes()


# ---- many launches in one arena ------------------------------------------------------------------------------------------------
ARENA_GUARD = 256      # bytes of fill in front of every range of an arena, and behind the last
FILL = 0xA5


def up256(x):
    return (x + 255) & ~255


class Arena:
    """Byte ranges at chosen residues (0..255) of a 256-byte aligned buffer, ARENA_GUARD or more fill bytes around each"""

    def __init__(self):
        self.at = 0

    def place(self, residue, nbytes):
        assert 0 <= residue < 256
        off = up256(self.at + ARENA_GUARD) + residue
        self.at = off + nbytes
        return off

    def size(self):
        return up256(self.at + ARENA_GUARD) + 256


# One buffer of `total` pixels, interleaved side at residue `i`, transformed side at residue `t`.  `pieces` None: one whole-buffer
# call; else the (first, num) range calls issued in that order into the one output.  `src` is what the call reads (all of the
# buffer: pixels forward, transformed bytes inverse), `want` the image of the whole output afterwards (FILL where no call of the job
# may write), `tag` what a failure says.
Job = collections.namedtuple("Job", "inverse B decorrelate layout total pieces src t i want tag")


def check_image(got, placed, label):
    """placed: [(offset, expected bytes, tag)] in arena order.  Every range equals its expectation and every other byte of the
    arena still holds FILL: one comparison with the expected image; what follows only words the failure."""
    image = np.full(got.size, FILL, dtype=np.uint8)
    for off, want, _ in placed:
        image[off:off + want.size] = want
    if np.array_equal(got, image):
        return
    for off, want, tag in placed:
        part = got[off:off + want.size]
        if not np.array_equal(part, want):
            bad = np.nonzero(part != want)[0]
            raise AssertionError(f"{label}: {bad.size} of {want.size} bytes differ, first at byte {int(bad[0])} "
                                 f"(got {int(part[bad[0]])}, want {int(want[bad[0]])}): case {tag}")
    stray = np.nonzero(got != image)[0]
    k = max(0, bisect.bisect_right([off for off, _, _ in placed], int(stray[0])) - 1)
    off, want, tag = placed[k]
    raise AssertionError(f"{label}: {stray.size} guard bytes changed, first at arena byte {int(stray[0])}; the output in front of it "
                         f"is [{off}, {off + want.size}): case {tag}")


def device_arena(dev, host):
    """the host image of an arena on the device"""
    import torch

    t = torch.from_numpy(host).to(dev)
    assert t.data_ptr() % 256 == 0, "the residues are taken from 256-byte aligned allocations"
    return t


def run_jobs(lib, dev, jobs, stream=None):
    """All sources in one arena (one per distinct (array, residue)), all outputs in another between guard bytes; every launch
    issued, one synchronise, one download of each arena.  Asserts: every status OK, every output == its `want`, every guard byte
    and every byte of the source arena unchanged."""
    import torch

    a_src, a_out = Arena(), Arena()
    src_at, out_at = {}, []
    for j in jobs:
        assert j.src.size == j.total * j.B == j.want.size, j.tag
        key = (id(j.src), j.t if j.inverse else j.i)
        if key not in src_at:
            src_at[key] = (a_src.place(key[1], j.src.size), j.src)
        out_at.append(a_out.place(j.i if j.inverse else j.t, j.want.size))
    h_src = np.full(a_src.size(), 0x3C, dtype=np.uint8)
    for off, data in src_at.values():
        h_src[off:off + data.size] = data
    d_src, d_out = device_arena(dev, h_src), device_arena(dev, np.full(a_out.size(), FILL, dtype=np.uint8))
    whole = (lib.dxtlt_transform_pixels_device, lib.dxtlt_untransform_pixels_device)
    ranged = lib.dxtlt_transform_pixels_range_device
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        for j, o in zip(jobs, out_at):
            src = d_src.data_ptr() + src_at[(id(j.src), j.t if j.inverse else j.i)][0]
            dst = d_out.data_ptr() + o
            if j.pieces is None:
                rc = whole[j.inverse](src, dst, j.total * j.B, j.B, j.decorrelate, j.layout, s)
                assert rc == OK, (rc, j.tag)
                continue
            for first, num in j.pieces:
                # the interleaved-side pointer is the range's first pixel, the transformed-side pointer byte 0 of the whole buffer
                rc = ranged(j.B, j.inverse, src if j.inverse else src + first * j.B, dst + first * j.B if j.inverse else dst,
                            j.total, first, num, j.decorrelate, j.layout, s)
                assert rc == OK, (rc, first, num, j.tag)
        torch.cuda.synchronize()
    got_out, got_src = d_out.cpu().numpy(), d_src.cpu().numpy()
    check_image(got_out, [(o, j.want, j.tag) for j, o in zip(jobs, out_at)], "output")
    assert np.array_equal(got_src, h_src), "a call changed its source arena"


def both_directions(x, want, B, decorrelate, layout, t, i, tag=()):
    """the two whole-buffer jobs of one buffer: forward of `x` == `want`, inverse of `want` == `x`"""
    total = x.size // B
    return [Job(False, B, decorrelate, layout, total, None, x, t, i, want, ("forward", total, B, decorrelate, layout, t, i) + tuple(tag)),
            Job(True, B, decorrelate, layout, total, None, want, t, i, x, ("inverse", total, B, decorrelate, layout, t, i) + tuple(tag))]


# ---- the combination draw ------------------------------------------------------------------------------------------------------
COUNT_KINDS = ("tiny", "segments +- 17", "any", "vectors +- a few")
DATA_KINDS = ("uniform", "walk", "constant", "alternating")
FuzzCase = collections.namedtuple("FuzzCase", "B decorrelate layout count_kind P in_off out_off cut data_kind data_seed")


def pick_count(rng):
    """four kinds, as pick_count of tests/test_gpu_fuzz.py: tiny; k * 4096 +- 17; anything up to 70 000; multiples of 16 +- a few"""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return kind, int(rng.integers(0, 70))
    if kind == 1:
        return kind, int(rng.integers(1, 18)) * R.SEGMENT + int(rng.integers(-17, 18))
    if kind == 2:
        return kind, int(rng.integers(1, 70_001))
    return kind, int(rng.integers(1, 300)) * 16 + int(rng.integers(-3, 4))


def draw_case(rng):
    """One case: B x settings x count x both pointer offsets (interleaved side, transformed side; three in five are 0) x whole
    buffer or two ranges cut on a multiple of 4096 (one in three of the buffers longer than a segment; cut 0 = whole) x data kind"""
    B = (3, 4)[int(rng.integers(0, 2))]
    decorrelate, layout = R.SETTINGS[int(rng.integers(0, len(R.SETTINGS)))]
    kind, P = pick_count(rng)
    offs = [0 if rng.integers(0, 5) < 3 else int(rng.integers(1, 128)) for _ in range(2)]
    cut = 0
    if rng.integers(0, 3) == 0 and P > R.SEGMENT:
        cut = R.SEGMENT * int(rng.integers(1, (P - 1) // R.SEGMENT + 1))
    return FuzzCase(B, decorrelate, layout, COUNT_KINDS[kind], P, offs[0], offs[1], cut, DATA_KINDS[int(rng.integers(0, 4))],
                    int(rng.integers(0, 1 << 31)))


def case_pixels(c):
    """the case's P * B input bytes"""
    rng = np.random.default_rng(c.data_seed)
    if c.data_kind == "uniform":
        px = rng.integers(0, 256, (c.P, c.B), dtype=np.uint8)
    elif c.data_kind == "walk":                       # steps in -2..2 per channel, modulo 256
        steps = rng.integers(-2, 3, (c.P, c.B))
        px = ((rng.integers(0, 256, c.B) + np.cumsum(steps, axis=0)) & 0xFF).astype(np.uint8)
    elif c.data_kind == "constant":
        px = np.tile(rng.integers(0, 256, c.B, dtype=np.uint8), (c.P, 1))
    else:                                             # 0 / 255 from pixel to pixel, the channels in opposite phase
        px = (255 * ((np.arange(c.P)[:, None] + np.arange(c.B)[None, :]) & 1)).astype(np.uint8)
    return np.ascontiguousarray(px).reshape(-1)


def case_jobs(c, index):
    """forward == reference, inverse of the reference's output == input; ranged cases issue the inverse pieces in the other order"""
    x = case_pixels(c)
    want = R.forward(x, c.B, c.decorrelate, c.layout)
    pieces = None if c.cut == 0 else [(0, c.cut), (c.cut, c.P - c.cut)]
    tag = (index,) + tuple(c)
    return [Job(False, c.B, c.decorrelate, c.layout, c.P, pieces, x, c.out_off, c.in_off, want, ("forward",) + tag),
            Job(True, c.B, c.decorrelate, c.layout, c.P, pieces and pieces[::-1], want, c.out_off, c.in_off, x, ("inverse",) + tag)]
