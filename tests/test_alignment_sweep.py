"""Every stream-base alignment of the BC1..BC5 tile kernels, on the device, under byte comparison.

plan_launches (csrc/bcn_kernels.hip) picks a kernel form from the byte address of every SoA stream: aligned tiles, forward halo
tiles (shift = base & 63) or inverse shifted tiles (base & 15), the natural or the generic LDS access form, the halo width, full
tiles and / or an edge workgroup.  tests/test_transform_plan.py pins that choice; this file runs what was chosen.  One function,
build_cases, lists (format, settings, direction, SoA residue p in 0..127, AoS residue a, total_blocks, first_block, num_blocks);
a test without a device proves through dxtlt_debug_plan_transform that the list reaches every shift of stream 0, both LDS forms
with and without full tiles and a tail workgroup, every halo width the planner can emit and every launch kind; three device
sweeps then run the list through the single-buffer call, the range call and the batch call with guard bytes around every output.

Expected bytes are the CPU statements (oracle.transform for BC1..BC3, bc45_ref for BC4 / BC5); they do not depend on a residue and
are computed once per (format, settings, block count).

Block counts, with T the edge-tile block count (lanes x 16 / block bytes): 1, 17, T - 1, T + 1, 2T + 9, 3T, 3T + 16 at every
residue 0..127 for the default settings and the all-off combination -- a sub-tile range, exactly one tail, full tiles plus a tail,
full tiles only --, 17, T + 1, 2T + 9, 3T at the 21 chosen residues for every other combination (counts_for_tile), and
T + 128 at residue 0 alone: with whole buffers the aligned tiles need every off_i * n on a 128-byte line, which of the seven counts
only 3T satisfies, so without T + 128 no case would run aligned tiles FOLLOWED by an edge tile.  BC1 without the colour split has
128-lane forward and 256-lane inverse tiles: its list holds the counts of both T, so that both directions run the same buffers.
"""
import bisect
import collections
import ctypes as C

import numpy as np
import pytest

import bc45_ref
from helpers import all_settings, pkg_settings
from test_batch_plan import Planned
from test_transform_plan import Launch, shift_lanes, streams as bc123_streams

FORMATS = ("bc1", "bc2", "bc3", "bc4", "bc5")
FMT_ID = {"bc1": 1, "bc2": 2, "bc3": 3, "bc4": 4, "bc5": 5}
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16, "bc4": 8, "bc5": 16}

# (variant, split_alpha, split_colour); BC4 / BC5 have one switch, split_endpoints, which travels as split_alpha
SETTINGS = {f: list(all_settings(f)) for f in ("bc1", "bc2", "bc3")}
SETTINGS.update({"bc4": [(0, 0, 0), (0, 1, 0)], "bc5": [(0, 0, 0), (0, 1, 0)]})
DEFAULT = {"bc1": (1, 0, 1), "bc2": (1, 0, 1), "bc3": (1, 1, 1), "bc4": (0, 0, 0), "bc5": (0, 0, 0)}
ALL_OFF = (0, 0, 0)
# all of 0..127 for the default settings and the all-off combination; BC4 / BC5 have two combinations and their default IS all-off,
# so both get every residue
FULL = {f: {DEFAULT[f], ALL_OFF} for f in ("bc1", "bc2", "bc3")}
FULL.update({"bc4": set(SETTINGS["bc4"]), "bc5": set(SETTINGS["bc5"])})
SUBSET = (0, 1, 2, 3, 6, 7, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 80, 96, 112, 127)
AOS_RESIDUES = (0, 1, 3, 4, 8, 12, 15)
RANGE_ORDER = (3, 0, 4, 1, 2)      # the order in which the five pieces of a range buffer are issued

GUARD = 256                        # bytes between two outputs of an arena and at its ends (the issue asks for 192 or more)
SOA_BASE, AOS_BASE = 0x7F00_0000_0000, 0x7F40_0000_0000    # stand-ins for a device allocation (the plan reads addresses mod 128)

Case = collections.namedtuple("Case", "fmt settings inverse p a total first num")


def fmt_streams(fmt, s):
    """[(offset, width)] in bytes per block of the SoA streams"""
    return bc45_ref.streams(fmt, bool(s[1])) if fmt in ("bc4", "bc5") else bc123_streams(FMT_ID[fmt], s[1], s[2])


def edge_blocks(fmt, s, inverse):
    return shift_lanes(FMT_ID[fmt], inverse, s[2]) * 16 // BLOCK[fmt]


def tiles_of(fmt, s):
    """the edge-tile block counts of the two directions (they differ for BC1 without the colour split only)"""
    return sorted({edge_blocks(fmt, s, False), edge_blocks(fmt, s, True)})


def counts_for_tile(fmt, s, T):
    """all seven counts where every residue runs; four of them -- a sub-tile range, one full tile and a tail of one block, full
    tiles plus a tail, full tiles only -- for the other settings combinations, whose address arithmetic is that of a full group
    with the same splits: this keeps each sweep below the time of the every-n test of its format"""
    return (1, 17, T - 1, T + 1, 2 * T + 9, 3 * T, 3 * T + 16) if s in FULL[fmt] else (17, T + 1, 2 * T + 9, 3 * T)


def counts_of(fmt, s):
    return sorted({n for T in tiles_of(fmt, s) for n in counts_for_tile(fmt, s, T)})


def aligned_extra(fmt, s):
    return tiles_of(fmt, s)[-1] + 128


def range_total_and_cuts(fmt, s):
    T = tiles_of(fmt, s)[-1]
    total = 5 * T + 9
    return total, [0, 1, T + 2, 3 * T, 3 * T + 16, total]


def residues_of(fmt, s):
    return tuple(range(128)) if s in FULL[fmt] else SUBSET


def halo_extra_count(fmt, s):
    """3T: off_i * 3T is a multiple of 64 for every stream, so every stream's shift is the pointer's and the halo is as wide as the
    narrowest stream makes it at that residue"""
    return 3 * tiles_of(fmt, s)[-1]


def halo_extra_residues(fmt, s):
    """BC3 with one of its two splits has no group that runs every residue, and the 21 chosen ones do not reach every halo width
    those stream layouts can ask for: the first settings combination of such a (split_alpha, split_colour) also runs the
    count 3T at every other residue."""
    splits = s[1:]
    if any(f[1:] == splits for f in FULL[fmt]) or s != next(x for x in SETTINGS[fmt] if x[1:] == splits):
        return ()
    return tuple(p for p in range(128) if p not in SUBSET)


def aos_residue(i):
    """a fixed function of the index: the second term keeps it from locking to the block count (seven counts, seven residues)"""
    return AOS_RESIDUES[(i + i // 7) % 7]


def build_cases(fmt):
    """Whole buffers (first_block 0, num_blocks == total_blocks), then the pieces of the range buffers (one AoS residue per buffer)"""
    out = []
    for s in SETTINGS[fmt]:
        for inverse in (False, True):
            i = 0
            for p in residues_of(fmt, s):
                for n in counts_of(fmt, s):
                    out.append(Case(fmt, s, inverse, p, aos_residue(i), n, 0, n))
                    i += 1
            n = aligned_extra(fmt, s)
            out.append(Case(fmt, s, inverse, 0, aos_residue(i), n, 0, n))
            for p in halo_extra_residues(fmt, s):
                i += 1
                out.append(Case(fmt, s, inverse, p, aos_residue(i), halo_extra_count(fmt, s), 0, halo_extra_count(fmt, s)))
            total, cuts = range_total_and_cuts(fmt, s)
            pieces = list(zip(cuts, cuts[1:]))
            for k, p in enumerate(residues_of(fmt, s)):
                for j in RANGE_ORDER:
                    out.append(Case(fmt, s, inverse, p, aos_residue(k), total, pieces[j][0], pieces[j][1] - pieces[j][0]))
    return out


_CASES = {}


def cases_of(fmt):
    if fmt not in _CASES:
        _CASES[fmt] = build_cases(fmt)
    return _CASES[fmt]


def is_whole(c):
    return c.first == 0 and c.num == c.total


_GROUPS = {}


def group_of(fmt, s, inverse, whole):
    """the cases of one (settings, direction): the whole buffers or the range pieces, in list order"""
    if fmt not in _GROUPS:
        g = collections.defaultdict(list)
        for c in cases_of(fmt):
            g[(c.settings, c.inverse, is_whole(c))].append(c)
        _GROUPS[fmt] = g
    return _GROUPS[fmt][(s, inverse, whole)]


@pytest.fixture(scope="module")
def lib(pkg):
    """the planner hooks of the library (no device needed), bound as tests/test_transform_plan.py and test_batch_plan.py bind them"""
    l = C.CDLL(pkg._lib.lib_path())
    l.dxtlt_debug_plan_transform.restype = C.c_int32
    l.dxtlt_debug_plan_transform.argtypes = [C.c_int32] * 5 + [C.c_uint64] * 5 + [C.c_void_p, C.c_int32]
    l.dxtlt_debug_plan_batch.restype = C.c_uint32
    l.dxtlt_debug_plan_batch.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return l


def plan_of(lib, c, soa_address=None, aos_address=None):
    """the planner's launches for a case; the addresses default to stand-ins with the case's residues"""
    soa = SOA_BASE + c.p if soa_address is None else soa_address
    aos = AOS_BASE + c.a + c.first * BLOCK[c.fmt] if aos_address is None else aos_address
    src, dst = (soa, aos) if c.inverse else (aos, soa)
    out = (Launch * 8)()
    v, sa, sc = c.settings
    n = lib.dxtlt_debug_plan_transform(FMT_ID[c.fmt], int(c.inverse), v, sa, sc, src, dst, c.total, c.first, c.num, out, 8)
    assert 0 < n <= 8, (c, n)
    return list(out)[:n]


def record(lib, c, soa_address=None, aos_address=None):
    """what an assertion message says about a case"""
    ns = len(fmt_streams(c.fmt, c.settings))
    launches = [dict(kind=l.kind, threads=l.threads, workgroups=l.workgroups, full_tiles=l.full_tiles, shift=list(l.shift)[:ns],
                     natural=l.natural, halo_vecs=l.halo_vecs) for l in plan_of(lib, c, soa_address, aos_address)]
    return (f"{c.fmt} v{c.settings[0]}-sa{c.settings[1]}-sc{c.settings[2]} {'inverse' if c.inverse else 'forward'} n={c.num} p={c.p} "
            f"a={c.a} total={c.total} first={c.first} plan={launches}")


# ------------------------------------------------------------------------------------------------------------
# 1. the case list and its coverage proof (no device)
# ------------------------------------------------------------------------------------------------------------
def planner_reach(lib, fmt):
    """What the forward planner can emit at all: p in 0..127 x n in 1..4T for every (split_alpha, split_colour) -- the planner
    reads the variant only to validate it -- as the set of halo_vecs of each (split_alpha, split_colour) and the set of
    (natural, tail workgroup) pairs."""
    halo, nat_tail = collections.defaultdict(set), set()
    out = (Launch * 4)()
    f = lib.dxtlt_debug_plan_transform
    for sa, sc in sorted({(s[1], s[2]) for s in SETTINGS[fmt]}):
        T = edge_blocks(fmt, (0, sa, sc), False)
        for p in range(128):
            for n in range(1, 4 * T + 1):
                cnt = f(FMT_ID[fmt], 0, 0, sa, sc, AOS_BASE, SOA_BASE + p, n, 0, n, out, 4)
                for l in out[:cnt]:
                    if l.kind:
                        halo[(sa, sc)].add(l.halo_vecs)
                        nat_tail.add((l.natural, l.workgroups > l.full_tiles))
    return halo, nat_tail


@pytest.mark.parametrize("fmt", FORMATS)
def test_case_list_reaches_every_kernel_form(lib, fmt):
    """The condition that keeps the list honest: thin it and this fails, on a machine without a GPU.

    One combination cannot occur and is asserted to be outside the planner's reach instead: forward, natural = 0 WITHOUT a tail
    workgroup -- natural = 0 needs a shift that is no multiple of its stream's element width, so a non-zero shift, and a forward
    launch with any non-zero shift always has the tail workgroup that writes the last d_s bytes of every stream."""
    cases = cases_of(fmt)
    for s in SETTINGS[fmt]:
        for inverse in (False, True):
            group = [c for c in cases if c.settings == s and c.inverse == inverse]
            whole = [c for c in group if is_whole(c)]
            res = set(range(128)) if s in FULL[fmt] else set(SUBSET)
            for T in tiles_of(fmt, s):
                for n in counts_for_tile(fmt, s, T):
                    extra = set(halo_extra_residues(fmt, s)) if n == halo_extra_count(fmt, s) else set()
                    assert {c.p for c in whole if c.num == n} == res | extra, (fmt, s, inverse, n)
            assert {c.p for c in group if not is_whole(c)} == res
            assert [c.a for c in whole] == [aos_residue(i) for i in range(len(whole))]
            total, cuts = range_total_and_cuts(fmt, s)
            assert {(c.first, c.first + c.num) for c in group if not is_whole(c)} == set(zip(cuts, cuts[1:]))
            assert any(f % 2 for f in cuts[1:-1]) and any(f % 2 == 0 and f % 16 for f in cuts[1:-1]) and any(
                f % tiles_of(fmt, s)[-1] == 0 for f in cuts[1:-1])
    assert FULL[fmt] <= set(SETTINGS[fmt]) and DEFAULT[fmt] in FULL[fmt] and ALL_OFF in FULL[fmt]

    reach_halo, reach_nat_tail = planner_reach(lib, fmt)
    assert (0, False) not in reach_nat_tail                   # the combination the docstring excludes
    for inverse in (False, True):
        shift0, nat_full, nat_tail, kinds, aos_nat = set(), set(), set(), set(), set()
        halo = collections.defaultdict(set)
        six_apart = False
        for c in cases:
            if c.inverse != inverse:
                continue
            launches = plan_of(lib, c)
            ns = len(fmt_streams(fmt, c.settings))
            if [l.kind for l in launches][:2] == [0, 2 if inverse else 1] and launches[1].full_tiles == 0:
                kinds.add("aligned tiles then an edge tile")
            for l in launches:
                if l.kind == 0:
                    continue
                assert l.kind == (2 if inverse else 1)
                shift0.add(l.shift[0])
                nat_full.add((l.natural, l.full_tiles > 0))
                nat_tail.add((l.natural, l.workgroups > l.full_tiles))
                halo[c.settings[1:]].add(l.halo_vecs)
                if launches[0].kind != 0:      # (an edge tile behind aligned tiles has no full tile either: counted above)
                    kinds.add("full tiles" if l.full_tiles else "no full tile")
                aos_nat.add((c.a, l.natural))
                six_apart = six_apart or (ns == 6 and len(set(list(l.shift)[:6])) == 6)
        tag = (fmt, "inverse" if inverse else "forward")
        assert shift0 == set(range(16 if inverse else 64)), (tag, sorted(set(range(64)) - shift0))
        assert nat_full == {(0, False), (0, True), (1, False), (1, True)}, (tag, nat_full)
        assert nat_tail == ({(0, False), (0, True), (1, False), (1, True)} if inverse else {(0, True), (1, False), (1, True)}), (tag, nat_tail)
        for splits, reach in reach_halo.items():     # per stream layout, not pooled: each must reach its own widths
            assert halo[splits] == (reach if not inverse else {0}), (tag, splits, sorted(reach - halo[splits]))
        assert kinds == {"aligned tiles then an edge tile", "full tiles", "no full tile"}, (tag, kinds)
        assert aos_nat == {(a, nat) for a in AOS_RESIDUES for nat in (0, 1)}, (tag, sorted(aos_nat))
        if fmt == "bc3":
            assert six_apart, (tag, "no case with both splits whose six streams have pairwise different shifts")


def stays_in_the_batch_kernel(lib, c):
    """Does the batch call keep this whole-buffer item in its own kernel?  (plan_batch_entry, csrc/batch_kernels.hip, hands an item
    whose shifts are not natural back to the single-buffer path.)"""
    soa, aos = SOA_BASE + c.p, AOS_BASE + c.a
    src, dst = (soa, aos) if c.inverse else (aos, soa)
    one = lambda v: (C.c_uint64 * 1)(v)
    out, index, wide = (Planned * 1)(), (C.c_uint8 * 4096)(), C.c_uint32(0)
    v, sa, sc = c.settings
    total = lib.dxtlt_debug_plan_batch(FMT_ID[c.fmt], int(c.inverse), v, sa, sc, one(src), one(dst), one(c.num), 1, out, index, 4096,
                                       C.byref(wide))
    return (out[0] if total != 0xFFFFFFFF else None)


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_sweep_runs_the_batch_kernel_where_shifts_are_natural(lib, fmt):
    """The batch kernel proper runs the items whose every shift is a multiple of its stream's element width; the others leave the
    batch call through the single-buffer path.  Which items stay is stated here independently and compared with the batch planner
    item by item, so that a change which hands everything back is noticed; the items that stay reach, per direction, every
    stream-0 shift the element widths allow, both tile forms, and buffers with and without full tiles."""
    for inverse in (False, True):
        mask = 15 if inverse else 63
        shift0, forms, full = set(), set(), set()
        for s in SETTINGS[fmt]:
            S = fmt_streams(fmt, s)
            items = group_of(fmt, s, inverse, True)
            kept = 0
            for c in items:
                d = [(c.p + off * c.num) & mask for off, w in S]
                natural = all(x % (2 if w == 6 else w) == 0 for (off, w), x in zip(S, d))
                e = stays_in_the_batch_kernel(lib, c)
                assert (e is not None) == natural, record(lib, c)
                if e is not None:
                    kept += 1
                    assert list(e.shift)[:len(S)] == d, record(lib, c)
                    shift0.add(d[0]); forms.add(e.form); full.add(e.full_tiles > 0)
            # the widest element of every layout here is 4 bytes or less: one residue in four at the least keeps 3T in the kernel
            assert len(items) // 32 <= kept < len(items), (fmt, s, inverse, kept, len(items))
        widest = max((2 if w == 6 else w) for s in SETTINGS[fmt] for off, w in fmt_streams(fmt, s))
        assert shift0 >= {x for x in range(mask + 1) if x % widest == 0}, (fmt, inverse, sorted(shift0))
        assert forms == {0, 1} and full == {False, True}, (fmt, inverse, forms, full)


# ------------------------------------------------------------------------------------------------------------
# device sweeps
# ------------------------------------------------------------------------------------------------------------
_STATEMENTS = {}


def statement(oracle, fmt, s, n):
    """(input blocks, their transform by the CPU statement), computed once per (format, settings, block count), read-only"""
    key = (fmt, s, n)
    if key not in _STATEMENTS:
        if ("pool", fmt) not in _STATEMENTS:
            _STATEMENTS[("pool", fmt)] = oracle.fill_splitmix64((5 * 512 + 9 + 64) * BLOCK[fmt], 0xA116E000 + FMT_ID[fmt])
        B = BLOCK[fmt]
        x = _STATEMENTS[("pool", fmt)][(n % 64) * B:(n % 64 + n) * B].copy()
        v, sa, sc = s
        want = bc45_ref.transform(fmt, x, bool(sa)) if fmt in ("bc4", "bc5") else oracle.transform(fmt, x, v, bool(sc), bool(sa))
        want = np.ascontiguousarray(want)
        x.setflags(write=False)
        want.setflags(write=False)
        _STATEMENTS[key] = (x, want)
    return _STATEMENTS[key]


def settings_object(pkg, fmt, s):
    if fmt in ("bc4", "bc5"):
        return (pkg.Bc4TransformSettings if fmt == "bc4" else pkg.Bc5TransformSettings)(bool(s[1]))
    return pkg_settings(pkg, fmt, s)


def up128(x):
    return (x + 127) & ~127


class Arena:
    """Byte ranges at chosen residues mod 128 inside one buffer, GUARD or more bytes between neighbours and at both ends"""

    def __init__(self):
        self.at, self.slots = 0, []

    def place(self, residue, nbytes, tag=None):
        off = up128(self.at + GUARD) + residue
        self.at = off + nbytes
        self.slots.append((off, nbytes, tag))
        return off

    def size(self):
        return up128(self.at + GUARD) + 128


@pytest.fixture(scope="module")
def dev():
    """the device with its context up, as the `dev` fixtures of the other device tests leave it"""
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    d = torch.device("cuda:0")
    torch.zeros(1, dtype=torch.uint8, device=d)
    torch.cuda.synchronize()
    return d


def device_arena(dev, size, fill):
    import torch

    t = torch.full((size,), fill, dtype=torch.uint8, device=dev)
    assert t.data_ptr() % 128 == 0, "the residues of this file are taken from a 128-byte aligned allocation"
    return t


def verify(lib, got, base_address, fill, placed, label, other_address):
    """placed: [(offset, expected bytes, case)].  Every range equals its expectation and every byte outside still holds `fill`:
    one comparison with the arena's expected image; what follows it only words the failure."""
    image = np.full(got.size, fill, dtype=np.uint8)
    for off, want, c in placed:
        image[off:off + want.size] = want
    if np.array_equal(got, image):
        return
    for off, want, c in placed:
        part = got[off:off + want.size]
        if not np.array_equal(part, want):
            bad = np.nonzero(part != want)[0]
            soa, aos = (other_address(c), base_address + off) if c.inverse else (base_address + off, other_address(c))
            pytest.fail(f"{label}: {bad.size} of {want.size} bytes differ, first at byte {int(bad[0])} (block {int(bad[0]) // BLOCK[c.fmt]}): "
                        f"{record(lib, c, soa, aos)}")
    stray = np.nonzero(got != image)[0]
    starts = [off for off, _, _ in placed]
    off, want, c = placed[max(0, bisect.bisect_right(starts, int(stray[0])) - 1)]
    pytest.fail(f"{label}: {stray.size} guard bytes changed, first at arena byte {int(stray[0])}; the output before it is "
                f"[{off}, {off + want.size}): {record(lib, c)}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_single_call_at_every_residue(pkg, oracle, lib, dev, fmt):
    """Every whole-buffer case through transform_{fmt}_with_settings and its inverse on slices of device tensors.  Per settings
    combination: all forward launches into one 0xA5 arena, all inverse launches -- reading the forward launches' own outputs, so
    what comes back is inverse(forward) -- into one 0x5A arena, then one download: forward == CPU statement, inverse == input,
    guards intact, inputs unchanged."""
    import torch

    B = BLOCK[fmt]
    forward, inverse = getattr(pkg, f"transform_{fmt}_with_settings"), getattr(pkg, f"untransform_{fmt}_with_settings")
    for s in SETTINGS[fmt]:
        st = settings_object(pkg, fmt, s)
        fwd, inv = group_of(fmt, s, False, True), group_of(fmt, s, True, True)
        a_in, a_fwd, a_inv = Arena(), Arena(), Arena()
        in_at = {}
        for c in fwd:
            if (c.num, c.a) not in in_at:
                in_at[(c.num, c.a)] = a_in.place(c.a, c.num * B)
        h_in = np.zeros(a_in.size(), dtype=np.uint8)
        for (n, a), off in in_at.items():
            h_in[off:off + n * B] = statement(oracle, fmt, s, n)[0]
        d_in = device_arena(dev, h_in.size, 0)
        d_in.copy_(torch.from_numpy(h_in))
        fwd_at = {(c.p, c.num): a_fwd.place(c.p, c.num * B) for c in fwd}
        inv_at = [a_inv.place(c.a, c.num * B) for c in inv]
        d_fwd, d_inv = device_arena(dev, a_fwd.size(), 0xA5), device_arena(dev, a_inv.size(), 0x5A)
        for c in fwd:
            i, o = in_at[(c.num, c.a)], fwd_at[(c.p, c.num)]
            forward(d_in[i:i + c.num * B], d_fwd[o:o + c.num * B], st)
        for c, o in zip(inv, inv_at):
            i = fwd_at[(c.p, c.num)]
            inverse(d_fwd[i:i + c.num * B], d_inv[o:o + c.num * B], st)
        torch.cuda.synchronize()
        got_fwd, got_inv, got_in = d_fwd.cpu().numpy(), d_inv.cpu().numpy(), d_in.cpu().numpy()
        verify(lib, got_fwd, d_fwd.data_ptr(), 0xA5, [(fwd_at[(c.p, c.num)], statement(oracle, fmt, s, c.num)[1], c) for c in fwd],
               "forward", lambda c: d_in.data_ptr() + in_at[(c.num, c.a)])
        verify(lib, got_inv, d_inv.data_ptr(), 0x5A, [(o, statement(oracle, fmt, s, c.num)[0], c) for c, o in zip(inv, inv_at)],
               "inverse", lambda c: d_fwd.data_ptr() + fwd_at[(c.p, c.num)])
        assert np.array_equal(got_in, h_in), (fmt, s, "a transform changed its input")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_range_calls_at_every_residue(pkg, oracle, lib, dev, fmt):
    """One whole buffer of 5T + 9 blocks per SoA residue, written by transform_range in five pieces whose first blocks are 0, odd,
    even but off 16, and tile-aligned, issued out of order: the shift vectors of the later pieces are non-natural BETWEEN streams,
    and every piece's head and tail bytes land inside lines its neighbours write.  Forward into one SoA buffer, inverse from it
    into one AoS buffer; same assertions as the single-call sweep."""
    import torch

    B = BLOCK[fmt]
    for s in SETTINGS[fmt]:
        st = settings_object(pkg, fmt, s)
        total, _ = range_total_and_cuts(fmt, s)
        x, want = statement(oracle, fmt, s, total)
        pieces = group_of(fmt, s, False, False) + group_of(fmt, s, True, False)
        a_in, a_fwd, a_inv = Arena(), Arena(), Arena()
        in_at = {a: a_in.place(a, total * B) for a in AOS_RESIDUES}
        h_in = np.zeros(a_in.size(), dtype=np.uint8)
        for off in in_at.values():
            h_in[off:off + total * B] = x
        d_in = device_arena(dev, h_in.size, 0)
        d_in.copy_(torch.from_numpy(h_in))
        fwd_at, inv_at, whole_of = {}, {}, {}
        for c in pieces:
            if c.p not in fwd_at:
                fwd_at[c.p], inv_at[c.p] = a_fwd.place(c.p, total * B), a_inv.place(c.a, total * B)
            whole_of.setdefault((c.p, c.inverse), c)
        d_fwd, d_inv = device_arena(dev, a_fwd.size(), 0xA5), device_arena(dev, a_inv.size(), 0x5A)
        for c in pieces:
            soa = d_fwd[fwd_at[c.p]:fwd_at[c.p] + total * B]
            if c.inverse:
                continue
            i = in_at[c.a] + c.first * B
            pkg.transform_range(fmt, False, d_in[i:i + c.num * B], soa, total, c.first, c.num, st)
        for c in pieces:
            soa = d_fwd[fwd_at[c.p]:fwd_at[c.p] + total * B]
            if not c.inverse:
                continue
            o = inv_at[c.p] + c.first * B
            pkg.transform_range(fmt, True, soa, d_inv[o:o + c.num * B], total, c.first, c.num, st)
        torch.cuda.synchronize()
        got_fwd, got_inv, got_in = d_fwd.cpu().numpy(), d_inv.cpu().numpy(), d_in.cpu().numpy()
        # a piece that differs is named: each piece's bytes of every stream forward, its blocks inverse
        for c in pieces:
            if c.inverse:
                o = inv_at[c.p] + c.first * B
                ok = np.array_equal(got_inv[o:o + c.num * B], x[c.first * B:(c.first + c.num) * B])
            else:
                ok = all(np.array_equal(got_fwd[fwd_at[c.p] + off * total + w * c.first:fwd_at[c.p] + off * total + w * (c.first + c.num)],
                                        want[off * total + w * c.first:off * total + w * (c.first + c.num)])
                         for off, w in fmt_streams(fmt, s))
            assert ok, "range piece differs: " + record(lib, c, d_fwd.data_ptr() + fwd_at[c.p],
                                                        (d_inv.data_ptr() + inv_at[c.p] if c.inverse else d_in.data_ptr() + in_at[c.a]) + c.first * B)
        verify(lib, got_fwd, d_fwd.data_ptr(), 0xA5, [(fwd_at[p], want, whole_of[(p, False)]) for p in fwd_at], "range forward",
               lambda c: d_in.data_ptr() + in_at[c.a])
        verify(lib, got_inv, d_inv.data_ptr(), 0x5A, [(inv_at[p], x, whole_of[(p, True)]) for p in inv_at], "range inverse",
               lambda c: d_fwd.data_ptr() + fwd_at[c.p])
        assert np.array_equal(got_in, h_in), (fmt, s, "a range call changed its input")


def pack(residues_and_sizes, first_gap):
    """Offsets of items packed side by side: 0..3 guard bytes behind each neighbour, then whatever reaches the item's residue"""
    at, offs = GUARD, []
    for k, (residue, nbytes) in enumerate(residues_and_sizes):
        at += (k + first_gap) % 4
        at += (residue - at) % 128
        offs.append(at)
        at += nbytes
    return offs, up128(at + GUARD) + 128


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_device_batch_at_every_residue(pkg, oracle, lib, dev, fmt):
    """ONE dxtlt_transform_batch_device call per settings combination and direction whose items are that group's whole-buffer cases,
    each at its exact SoA and AoS residue in one input and one output arena, 0..3 fill bytes (plus what reaches the residue) between
    neighbours.  The batch kernel proper takes the items whose shifts are natural (its per-item shift lookup at every such
    residue; test_batch_sweep_runs_the_batch_kernel_where_shifts_are_natural says which); the call hands the others to the
    single-buffer path, which this checks at the same packing.  Every item against the CPU statement, every byte between items against the fill."""
    import torch

    from dxt_lossless_transform_amd import batch

    B = BLOCK[fmt]
    for s in SETTINGS[fmt]:
        st = settings_object(pkg, fmt, s)
        for inverse, fill in ((False, 0xA5), (True, 0x5A)):
            items = group_of(fmt, s, inverse, True)
            data = [statement(oracle, fmt, s, c.num) for c in items]
            srcs, wants = ([w for _, w in data], [x for x, _ in data]) if inverse else ([x for x, _ in data], [w for _, w in data])
            in_offs, in_size = pack([(c.p if inverse else c.a, c.num * B) for c in items], 1)
            out_offs, out_size = pack([(c.a if inverse else c.p, c.num * B) for c in items], 0)
            h_in = np.zeros(in_size, dtype=np.uint8)
            for src, i in zip(srcs, in_offs):
                h_in[i:i + src.size] = src
            d_in = device_arena(dev, in_size, 0)
            d_in.copy_(torch.from_numpy(h_in))
            d_out = device_arena(dev, out_size, fill)
            batch.transform_batch([(fmt, inverse, d_in[i:i + c.num * B], d_out[o:o + c.num * B], st)
                                   for c, i, o in zip(items, in_offs, out_offs)])
            torch.cuda.synchronize()
            in_of = {id(c): i for c, i in zip(items, in_offs)}
            verify(lib, d_out.cpu().numpy(), d_out.data_ptr(), fill, list(zip(out_offs, wants, items)),
                   f"batch {'inverse' if inverse else 'forward'} (the record is the single-buffer planner's for these addresses)",
                   lambda c: d_in.data_ptr() + in_of[id(c)])
            assert np.array_equal(d_in.cpu().numpy(), h_in), (fmt, s, inverse, "the batch call changed its input")
