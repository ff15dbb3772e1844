"""The block-normalisation kernels at every pointer alignment and in every block slot, on the device, under byte comparison.

csrc/normalize_kernels.hip and the fused BC1 normalise+transform kernels of csrc/bcn_kernels.hip
(bc1_norm_kernels<VARIANT, SC, NORM>) choose their code from pointer alignment -- 16-byte vectors of two or four blocks, 4-byte
words, single bytes -- and, fused, from the byte address of every SoA stream as the plain tile kernels do.  tests/test_normalize*.py
pin WHAT they compute at aligned pointers; this file runs every one of those choices, with guard bytes around every output.

Expected bytes are the CPU statements of oracle/ (normalize_bc{1,2,3}_blocks, ..._split_blocks, ..._all_modes and
transform_bc1_with_normalize_blocks), which the reference's unit vectors pin in tests/test_normalize*.py.  Byte equality only.

0. Data.  crafted_blocks (tests/test_normalize.py) picks the case of block i by i % 8, and the vector paths put 2 or 4 blocks into
   one lane: there a case only ever sits in one half of the vector.  permuted_blocks draws the case from a seeded permutation; BC2 /
   BC3 take structured_blocks rows by class (alpha kept / uniform / uniform and opaque, colour kept / solid) the same way.  A test
   without a device asserts that every case occurs at every i % 4 and in both halves of every run of 64 blocks, for every block
   count of this file, and that the normalisation of such data differs from the data.
1. Fused BC1 normalise+transform: the BC1 forward whole-buffer cases of test_alignment_sweep.build_cases (all 128 SoA residues x
   seven counts for the default and the all-off settings, 21 residues x four counts for the other six), for both colour modes.
   plan_launches reads the addresses, the block counts and the two force bits; `normalize` enters only through
   aligned_tile_threads, where it makes a tuned tile size void (set_tuning(0, ...) leaves the default anyway).  So the plans that
   dxtlt_debug_plan_transform reports are the plans of the normalising call, and a test without a device shows that the list reaches
   every stream-0 shift, both LDS forms with and without full tiles and a tail workgroup, every halo width, aligned tiles followed
   by an edge tile -- and, for each of the eight (variant, split) kernel sets, all three launchable members (tiled, halo[0],
   halo[1]) without any force bit.  The forced forms (set_tuning(0, 2 | 0x20 | 0x22)) add what no address reaches: the issue's
   counts T + 1 and 2T + 9 never have all stream bases on a 128-byte line, so bit 2 alone changes nothing there; the count 3T at
   residues 0 and 64 does, and runs the natural AND the generic form on zero shifts with no tail workgroup -- the same test shows
   that under the debug planner.
   The internal mode 3 (transparent blocks only) has no device entry point of its own; it runs only inside
   dxtlt_transform_bc1_auto_with_normalization (part 4).
2. normalize_blocks of BC1 / BC2 / BC3 at all 81 (input, output) residue pairs of (0, 4, 8, 12, 1, 2, 3, 6, 15) and in place at
   each, block counts around one workgroup of single lanes (256) and of pair lanes (512).
3. The split-in-place and the all-modes kernels at misaligned arrays; arrays a mode does not touch stay byte-identical.
4. The "anything normalisable?" flag with exactly ONE normalisable block: first, last, odd tail, last lane of a wave, last partial
   wave; and the host call that is the only route to any_normalizable_kernel.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import oracle_auto
from test_alignment_sweep import (FULL, SETTINGS, SUBSET, Arena, aos_residue, build_cases, counts_for_tile, dev, device_arena,  # noqa: F401
                                  edge_blocks, group_of, is_whole, lib, plan_of, planner_reach, tiles_of, verify)
from test_alignment_sweep import Case
from test_normalize import permuted_blocks
from test_normalize_bc23 import structured_blocks

COLOR0, REPL = 1, 2
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16}
FUSED_SETTINGS = SETTINGS["bc1"]                       # (variant, 0, split_colour), eight of them
FORCED = (0x2, 0x20, 0x22)
FORCED_RESIDUES = (0, 1, 2, 6, 64)

R = (0, 4, 8, 12, 1, 2, 3, 6, 15)                      # both 16-aligned, 4 but not 16, not 4
COUNTS = (1, 2, 3, 5, 255, 256, 257, 511, 512, 513, 1025)
SPLIT_R = (0, 4, 8, 1, 2, 3)
BC1_SPLIT_COUNTS = COUNTS + (1023, 1024, 1027)         # a workgroup of four-block lanes is 1024 blocks
ALL_MODES_COUNTS = (1, 2, 3, 257, 513, 1025)
FLAG_COUNTS = (1, 2, 129, 513, 1025)
MODES = {"bc1": [(0, 1), (0, 2)], "bc2": [(0, 1), (0, 2)],
         "bc3": [(a, c) for a in range(4) for c in range(3) if (a, c) != (0, 0)]}      # (alpha mode, colour mode)


def forced_counts(s):
    T = edge_blocks("bc1", s, False)
    return (T + 1, 2 * T + 9, 3 * T)


def fused_counts():
    return sorted({c.num for s in FUSED_SETTINGS for c in group_of("bc1", s, False, True)} |
                  {n for s in FUSED_SETTINGS for n in forced_counts(s)})


def counts_used(fmt):
    own = set(COUNTS) | set(ALL_MODES_COUNTS)
    return sorted(own | set(BC1_SPLIT_COUNTS) | set(fused_counts()) if fmt == "bc1" else own)


# ------------------------------------------------------------------------------------------------------------
# 0. data whose cases do not depend on the slot
# ------------------------------------------------------------------------------------------------------------
RUNS = 5                                               # a count starts at run (n % RUNS) of its pool: small counts see different cases
_POOLS = {}


def class_table(fmt, oracle, rows):
    """the class of every structured_blocks row: 2 * alpha class + colour class; alpha 0 kept, 1 uniform, 2 uniform and opaque (the
    three alpha modes differ on these alone), colour 0 kept, 1 solid.  Read off the CPU statement."""
    flat = rows.reshape(-1)
    if fmt == "bc2":
        return (oracle.normalize_bc2_blocks(flat, COLOR0).reshape(-1, 16) != rows).any(axis=1).astype(np.int64), 2
    y1 = oracle.normalize_bc3_blocks(flat, 1, COLOR0).reshape(-1, 16)
    y2 = oracle.normalize_bc3_blocks(flat, 2, COLOR0).reshape(-1, 16)
    uniform, opaque = (y1[:, :8] != rows[:, :8]).any(axis=1), (y1 != y2).any(axis=1)
    colour = (y1[:, 8:] != rows[:, 8:]).any(axis=1)
    return 2 * np.where(opaque, 2, uniform.astype(np.int64)) + colour, 6


def classed_blocks(fmt, oracle, n, seed):
    """structured_blocks rows through a seeded shuffle that is blind to the slot: in every aligned run of 32 blocks the eight
    positions of each i % 4 hold every class once (the spare positions: any class), each position a random row of its class"""
    rng = np.random.default_rng(seed)
    rows = structured_blocks(fmt, rng).reshape(-1, 16)
    cls, count = class_table(fmt, oracle, rows)
    members = [np.flatnonzero(cls == k) for k in range(count)]
    assert all(m.size >= 8 for m in members), [m.size for m in members]
    want = np.empty((n + 31) // 32 * 32, dtype=np.int64)
    for run in want.reshape(-1, 8, 4):
        for slot in range(4):
            run[:, slot] = rng.permutation(np.concatenate([np.arange(count), rng.integers(0, count, 8 - count)]) if count < 8
                                           else np.arange(8))
    want = want[:n]
    pick = np.empty(n, dtype=np.int64)
    for k in range(count):
        at = np.flatnonzero(want == k)
        pick[at] = rng.choice(members[k], at.size)
    return np.ascontiguousarray(rows[pick].reshape(-1))


def pool(oracle, fmt):
    if fmt not in _POOLS:
        n = max(counts_used(fmt)) + 32 * RUNS
        if fmt == "bc1":
            x, k = permuted_blocks(oracle, n, 0xA11)
        else:
            x, k = classed_blocks(fmt, oracle, n, 0xBC23A11 + BLOCK[fmt]), None
        x.setflags(write=False)
        _POOLS[fmt] = (x, k)
    return _POOLS[fmt]


def blocks_of(oracle, fmt, n):
    """the n blocks every test of this file uses for that count (read-only)"""
    x, _ = pool(oracle, fmt)
    first = 32 * (n % RUNS)
    return x[first * BLOCK[fmt]:(first + n) * BLOCK[fmt]]


def cases_of_blocks(oracle, n):
    _, k = pool(oracle, "bc1")
    return k[32 * (n % RUNS):32 * (n % RUNS) + n]


_WANT = {}


def normalized(oracle, fmt, n, mode):
    """the CPU statement of normalize_blocks for blocks_of(fmt, n); mode = (alpha mode, colour mode).  Once per key, read-only."""
    key = (fmt, n, mode)
    if key not in _WANT:
        x, (a, c) = blocks_of(oracle, fmt, n), mode
        y = (oracle.normalize_bc1_blocks(x, c) if fmt == "bc1" else oracle.normalize_bc2_blocks(x, c) if fmt == "bc2"
             else oracle.normalize_bc3_blocks(x, a, c))
        y.setflags(write=False)
        _WANT[key] = y
    return _WANT[key]


def in_every_slot(mask):
    """does the property occur at every i % 4, and in both halves of every complete run of 64 blocks?"""
    whole = mask[:mask.size // 64 * 64].reshape(-1, 2, 32)
    return {int(i) % 4 for i in np.flatnonzero(mask)} == {0, 1, 2, 3} and bool(whole.any(axis=2).all())


def test_data_cases_are_independent_of_the_slot(oracle):
    for n in counts_used("bc1"):
        x, k = blocks_of(oracle, "bc1", n), cases_of_blocks(oracle, n)
        if n < 64:
            continue
        for case in range(8):
            assert in_every_slot(k == case), ("bc1", n, case)
        b = x.reshape(-1, 8)
        y1, y2 = normalized(oracle, "bc1", n, (0, COLOR0)).reshape(-1, 8), normalized(oracle, "bc1", n, (0, REPL)).reshape(-1, 8)
        assert not np.array_equal(y1, b) and not np.array_equal(y2, b) and not np.array_equal(y1, y2)
        # what the statement does with the cases, not only their labels: transparent, solid, kept
        transparent = (y1 == 0xFF).all(axis=1) & (b != 0xFF).any(axis=1)
        solid = (y1 != b).any(axis=1) & ~transparent
        for name, mask in (("transparent", transparent), ("solid", solid), ("kept", (y1 == b).all(axis=1))):
            assert in_every_slot(mask), ("bc1", n, name)
        # (cases 3 and 6 are solid in an interpolated colour, which the statement rewrites only where it survives 565 rounding)
        assert np.array_equal(transparent, k == 5) and solid[np.isin(k, (1, 2, 4))].all() and not solid[np.isin(k, (0, 7))].any()
    for fmt in ("bc2", "bc3"):
        for n in counts_used(fmt):
            if n < 64:
                continue
            b = blocks_of(oracle, fmt, n).reshape(-1, 16)
            for c in (COLOR0, REPL):
                y = normalized(oracle, fmt, n, (0, c)).reshape(-1, 16)
                assert in_every_slot((y[:, 8:] != b[:, 8:]).any(axis=1)), (fmt, n, "colour half changes", c)
                assert in_every_slot((y == b).all(axis=1)), (fmt, n, "kept")
                assert np.array_equal(y[:, :8], b[:, :8])
            if fmt == "bc3":
                ys = [normalized(oracle, fmt, n, (a, 0)).reshape(-1, 16) for a in (1, 2, 3)]
                for a, y in zip((1, 2, 3), ys):
                    assert in_every_slot((y[:, :8] != b[:, :8]).any(axis=1)), (fmt, n, "alpha half changes", a)
                    assert np.array_equal(y[:, 8:], b[:, 8:])
                for p, q in itertools.combinations(ys, 2):      # opaque uniform blocks: where the three alpha modes part
                    assert in_every_slot((p != q).any(axis=1)), (fmt, n, "opaque uniform alpha")


# ------------------------------------------------------------------------------------------------------------
# 1. fused BC1 normalise+transform
# ------------------------------------------------------------------------------------------------------------
_FUSED = {}


def fused_statement(oracle, s, n, mode):
    """(input blocks, oracle.transform_bc1_with_normalize_blocks of them), once per key, read-only.  From 17 blocks on the
    expectation is not the plain transform of the input: a kernel that forgot to normalise fails."""
    key = (s, n, mode)
    if key not in _FUSED:
        x = blocks_of(oracle, "bc1", n)
        want = np.ascontiguousarray(oracle.transform_bc1_with_normalize_blocks(x, mode, s[0], bool(s[2])))
        if n >= 17:
            assert not np.array_equal(want, oracle.transform("bc1", x, s[0], bool(s[2]))), key
        want.setflags(write=False)
        _FUSED[key] = (x, want)
    return _FUSED[key]


def forced_cases(s):
    out = []
    for n in forced_counts(s):
        for p in FORCED_RESIDUES:
            out.append(Case("bc1", s, False, p, aos_residue(len(out)), n, 0, n))
    return out


def test_fused_case_list_reaches_every_kernel_form(pkg, lib, oracle):
    """No device.  The cases the fused sweep runs are the BC1 forward whole-buffer cases of the plain sweep; what
    test_case_list_reaches_every_kernel_form[bc1] shows for the whole list is shown here for that subset, then per kernel set, then
    for the forced forms."""
    whole = [c for c in build_cases("bc1") if not c.inverse and is_whole(c)]
    assert whole == [c for s in FUSED_SETTINGS for c in group_of("bc1", s, False, True)]
    for s in FUSED_SETTINGS:
        group = group_of("bc1", s, False, True)
        res = set(range(128)) if s in FULL["bc1"] else set(SUBSET)
        for T in tiles_of("bc1", s):
            for n in counts_for_tile("bc1", s, T):
                assert {c.p for c in group if c.num == n} == res, (s, n)
    assert (1, 0, 1) in FULL["bc1"] and (0, 0, 0) in FULL["bc1"]
    reach_halo, _ = planner_reach(lib, "bc1")
    pkg.set_tuning(0, 0)
    shift0, nat_full, nat_tail, kinds = set(), set(), set(), set()
    halo = {splits: set() for splits in reach_halo}
    members = {s: set() for s in FUSED_SETTINGS}
    for c in whole:
        launches = plan_of(lib, c)
        if [l.kind for l in launches][:2] == [0, 1] and launches[1].full_tiles == 0:
            kinds.add("aligned tiles then an edge tile")
        for l in launches:
            members[c.settings].add("tiled" if l.kind == 0 else f"halo[{l.natural}]")
            if l.kind == 0:
                continue
            assert l.kind == 1
            shift0.add(l.shift[0])
            nat_full.add((l.natural, l.full_tiles > 0))
            nat_tail.add((l.natural, l.workgroups > l.full_tiles))
            halo[c.settings[1:]].add(l.halo_vecs)
            if launches[0].kind != 0:
                kinds.add("full tiles" if l.full_tiles else "no full tile")
    assert shift0 == set(range(64)), sorted(set(range(64)) - shift0)
    assert nat_full == {(0, False), (0, True), (1, False), (1, True)}
    assert nat_tail == {(0, True), (1, False), (1, True)}         # (0, False) is outside the planner's reach without a force bit
    assert halo == reach_halo
    assert kinds == {"aligned tiles then an edge tile", "full tiles", "no full tile"}
    assert all(m == {"tiled", "halo[0]", "halo[1]"} for m in members.values()), members
    try:
        for s in FUSED_SETTINGS:
            seen = set()
            for f in FORCED:
                pkg.set_tuning(0, f)
                for c in forced_cases(s):
                    launches = plan_of(lib, c)
                    if f & 2:
                        assert [l.kind for l in launches] == [1], (s, f, c)
                    for l in launches:
                        if l.kind:
                            assert not (f & 0x20 and l.natural)
                            seen.add((f, l.natural, l.full_tiles > 0, l.workgroups > l.full_tiles, any(list(l.shift)[:3])))
            # bit 2 moves aligned buffers into the halo tiles, zero shifts and no tail workgroup, in both LDS forms
            assert (0x2, 1, True, False, False) in seen and (0x22, 0, True, False, False) in seen, (s, seen)
            # bit 0x20 runs the generic form on shifts the natural form would have taken
            assert all((f, 0, True, True, True) in seen for f in (0x20, 0x22)) and (0x2, 1, True, True, True) in seen, (s, seen)
    finally:
        pkg.set_tuning(0, 0)
    for mode in (COLOR0, REPL):                                    # the expectation is never the un-normalised transform
        for s in FUSED_SETTINGS:
            for n in sorted({c.num for c in group_of("bc1", s, False, True)} | set(forced_counts(s))):
                fused_statement(oracle, s, n, mode)


@pytest.fixture(scope="module")
def norm(pkg):
    from dxt_lossless_transform_amd import normalize as mod

    return mod


@pytest.fixture(scope="module")
def n23(pkg):
    from dxt_lossless_transform_amd import normalize23 as mod

    return mod


def run_fused(pkg, norm, oracle, lib, dev, mode, s, launches, label):
    """launches: [(case, force bits)], each into its own slot of one 0xA5 arena at the case's SoA residue, reading its input at the
    case's AoS residue; one download: outputs == CPU statement, guards intact, inputs unchanged"""
    import torch

    details = norm.Bc1TransformDetailsWithNormalization(norm.ColorNormalizationMode(mode), s[0], bool(s[2]))
    a_in, a_out = Arena(), Arena()
    in_at = {}
    for c, _ in launches:
        if (c.num, c.a) not in in_at:
            in_at[(c.num, c.a)] = a_in.place(c.a, c.num * 8)
    h_in = np.zeros(a_in.size(), dtype=np.uint8)
    for (n, a), off in in_at.items():
        h_in[off:off + n * 8] = fused_statement(oracle, s, n, mode)[0]
    d_in = device_arena(dev, h_in.size, 0)
    d_in.copy_(torch.from_numpy(h_in))
    out_at = [a_out.place(c.p, c.num * 8) for c, _ in launches]
    d_out = device_arena(dev, a_out.size(), 0xA5)
    force_now = 0
    try:
        for (c, f), o in zip(launches, out_at):
            if f != force_now:
                pkg.set_tuning(0, f)
                force_now = f
            i = in_at[(c.num, c.a)]
            norm.transform_bc1_with_normalize_blocks(d_in[i:i + c.num * 8], d_out[o:o + c.num * 8], details)
    finally:
        pkg.set_tuning(0, 0)
    torch.cuda.synchronize()
    got_out, got_in = d_out.cpu().numpy(), d_in.cpu().numpy()
    verify(lib, got_out, d_out.data_ptr(), 0xA5, [(o, fused_statement(oracle, s, c.num, mode)[1], c) for (c, _), o in zip(launches, out_at)],
           label, lambda c: d_in.data_ptr() + in_at[(c.num, c.a)])
    assert np.array_equal(got_in, h_in), (label, "the fused transform changed its input")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [COLOR0, REPL])
def test_fused_transform_at_every_residue(pkg, norm, oracle, lib, dev, mode):
    for s in FUSED_SETTINGS:
        run_fused(pkg, norm, oracle, lib, dev, mode, s, [(c, 0) for c in group_of("bc1", s, False, True)],
                  f"fused mode {mode} v{s[0]}-sc{s[2]}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [COLOR0, REPL])
def test_fused_transform_forced_forms(pkg, norm, oracle, lib, dev, mode):
    """halo tiles for aligned bases (2), the generic LDS form for natural shifts (0x20), both (0x22), for every kernel set"""
    for s in FUSED_SETTINGS:
        run_fused(pkg, norm, oracle, lib, dev, mode, s, [(c, f) for f in FORCED for c in forced_cases(s)],
                  f"fused mode {mode} v{s[0]}-sc{s[2]}, forced forms 0x2, 0x20, 0x22 in thirds (the plan shown is the unforced one)")


# ------------------------------------------------------------------------------------------------------------
# arenas of parts 2 to 4
# ------------------------------------------------------------------------------------------------------------
class Slots:
    """Byte ranges of one device allocation at chosen residues, guard bytes between them: what each holds before the calls (None:
    the fill) and what it has to hold after them (by default what it held before)."""

    def __init__(self, fill):
        self.fill, self.arena, self.items, self.t = fill, Arena(), [], None

    def add(self, residue, label, initial=None, nbytes=None, want=None):
        n = initial.size if initial is not None else nbytes
        self.items.append([self.arena.place(residue, n), n, initial, initial if want is None else want, label])
        return len(self.items) - 1

    def upload(self, dev):
        import torch

        h = np.full(self.arena.size(), self.fill, dtype=np.uint8)
        for off, n, initial, _, _ in self.items:
            if initial is not None:
                h[off:off + n] = initial
        self.t = device_arena(dev, h.size, self.fill)
        self.t.copy_(torch.from_numpy(h))
        return self

    def view(self, k):
        off, n = self.items[k][:2]
        return self.t[off:off + n]

    def check(self):
        """one download, one comparison with the expected image; the rest words the failure"""
        got = self.t.cpu().numpy()
        image = np.full(got.size, self.fill, dtype=np.uint8)
        for off, n, _, want, label in self.items:
            assert want is not None and want.size == n, label
            image[off:off + n] = want
        if np.array_equal(got, image):
            return
        for off, n, _, want, label in self.items:
            bad = np.flatnonzero(got[off:off + n] != want)
            if bad.size:
                i = int(bad[0])
                pytest.fail(f"{label}: {bad.size} of {n} bytes differ, first at byte {i}: got {got[off + i:off + min(i + 8, n)].tolist()}, "
                            f"want {want[i:i + 8].tolist()}")
        stray = np.flatnonzero(got != image)
        before = max((it for it in self.items if it[0] <= stray[0]), key=lambda it: it[0], default=self.items[0])
        pytest.fail(f"{stray.size} guard bytes changed, first at arena byte {int(stray[0])}; the range before it is "
                    f"[{before[0]}, {before[0] + before[1]}): {before[4]}")


# ------------------------------------------------------------------------------------------------------------
# 2. stand-alone normalize_blocks
# ------------------------------------------------------------------------------------------------------------
def call_normalize(norm, n23, fmt, src, dst, mode):
    a, c = mode
    if fmt == "bc1":
        norm.normalize_blocks(src, dst, norm.ColorNormalizationMode(c))
    else:
        n23.normalize_blocks(fmt, src, dst, n23.ColorNormalizationMode(c), n23.AlphaNormalizationMode(a))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bc1", "bc2", "bc3"])
def test_normalize_blocks_at_every_alignment_class(norm, n23, oracle, dev, fmt):
    """All 81 residue pairs and in place at all nine residues, per mode one arena and one download.  Mode None / (None, None) is
    the copy shortcut: one count at three pairs, and in place, where it must leave the buffer alone."""
    ins = Slots(0)
    in_at = {(n, r): ins.add(r, f"{fmt} input n={n} residue {r}", initial=blocks_of(oracle, fmt, n)) for n in COUNTS for r in R}
    ins.upload(dev)
    for mode in MODES[fmt] + [(0, 0)]:
        copy = mode == (0, 0)
        outs, calls = Slots(0xA5), []
        for n in ((257,) if copy else COUNTS):
            x, want = blocks_of(oracle, fmt, n), (blocks_of(oracle, fmt, n) if copy else normalized(oracle, fmt, n, mode))
            for ri, ro in (((0, 0), (4, 1), (3, 8)) if copy else itertools.product(R, R)):
                calls.append((in_at[(n, ri)], outs.add(ro, f"{fmt} mode {mode} n={n} in at {ri} out at {ro}", nbytes=x.size, want=want)))
            for r in ((0, 3) if copy else R):
                calls.append((None, outs.add(r, f"{fmt} mode {mode} n={n} in place at {r}", initial=x, want=want)))
        outs.upload(dev)
        for i, k in calls:
            dst = outs.view(k)
            call_normalize(norm, n23, fmt, dst if i is None else ins.view(i), dst, mode)
        outs.check()
    ins.check()


# ------------------------------------------------------------------------------------------------------------
# 3. split-in-place and all-modes
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bc1", "bc2"])
def test_split_in_place_at_misaligned_arrays(norm, n23, oracle, dev, fmt):
    """colours and indices each at (0, 4, 8, 1, 2, 3): the vector path (BC1), the word path, the byte path, and the mixed pairs"""
    B = BLOCK[fmt]
    for mode in (COLOR0, REPL):
        s, calls = Slots(0xA5), []
        for n in (BC1_SPLIT_COUNTS if fmt == "bc1" else COUNTS):
            b = blocks_of(oracle, fmt, n).reshape(-1, B)
            c, i = b[:, B - 8:B - 4].reshape(-1).copy(), b[:, B - 4:].reshape(-1).copy()
            if fmt == "bc1":
                wc, wi = oracle.normalize_bc1_split_blocks(c, i, mode)
            else:
                wc, wi = oracle.normalize_bc2_split_blocks(b[:, :8].reshape(-1).copy(), c, i, mode)
            if n >= 64:
                assert not np.array_equal(wc, c) and not np.array_equal(wi, i)
            for rc, ri in itertools.product(SPLIT_R, SPLIT_R):
                tag = f"{fmt} split mode {mode} n={n} colours at {rc} indices at {ri}"
                calls.append((s.add(rc, tag + ": colours", initial=c, want=wc), s.add(ri, tag + ": indices", initial=i, want=wi)))
        s.upload(dev)
        for kc, ki in calls:
            if fmt == "bc1":
                norm.normalize_split_blocks_in_place(s.view(kc), s.view(ki), norm.ColorNormalizationMode(mode))
            else:
                n23.normalize_bc2_split_blocks_in_place(None, s.view(kc), s.view(ki), n23.ColorNormalizationMode(mode))
        s.check()


BC3_ALPHA_R = list(itertools.product((0, 1), (0, 1, 2, 3)))                    # alpha endpoints x alpha indices
BC3_COLOUR_R = [(0, 0), (4, 4), (1, 1), (2, 2), (0, 2), (1, 4)]                # colour endpoints, colour indices: diagonal + two mixed


@pytest.mark.gpu
def test_bc3_split_in_place_at_misaligned_arrays(n23, oracle, dev):
    """Four arrays, each in its own guarded slot.  A mode whose alpha (colour) half is None must leave the two alpha (colour)
    arrays byte-identical: their expectation is the input itself."""
    for a, cm in MODES["bc3"]:
        s, calls = Slots(0xA5), []
        for n in COUNTS:
            b = blocks_of(oracle, "bc3", n).reshape(-1, 16)
            parts = [b[:, :2].reshape(-1).copy(), b[:, 2:8].reshape(-1).copy(), b[:, 8:12].reshape(-1).copy(), b[:, 12:].reshape(-1).copy()]
            want = oracle.normalize_bc3_split_blocks(*parts, a, cm)
            if a == 0:
                assert np.array_equal(want[0], parts[0]) and np.array_equal(want[1], parts[1])
                want[0], want[1] = parts[0], parts[1]
            if cm == 0:
                assert np.array_equal(want[2], parts[2]) and np.array_equal(want[3], parts[3])
                want[2], want[3] = parts[2], parts[3]
            if n >= 64:
                assert all(np.array_equal(w, p) == (mode_half == 0) for w, p, mode_half in zip(want, parts, (a, a, cm, cm)))
            for (rae, rai), (rce, rci) in itertools.product(BC3_ALPHA_R, BC3_COLOUR_R):
                tag = f"bc3 split mode ({a}, {cm}) n={n} arrays at {(rae, rai, rce, rci)}: "
                calls.append([s.add(r, tag + name, initial=p, want=w) for r, name, p, w in
                              zip((rae, rai, rce, rci), ("alpha endpoints", "alpha indices", "colour endpoints", "colour indices"), parts, want)])
        s.upload(dev)
        for ks in calls:
            n23.normalize_bc3_split_blocks_in_place(*[s.view(k) for k in ks], n23.AlphaNormalizationMode(a), n23.ColorNormalizationMode(cm))
        s.check()


def pointer_rounds(pointers, residues):
    """all at 0; each pointer in turn at each residue while the others sit at 0; all at 8; all at 1"""
    rounds = [(0,) * pointers]
    for r in residues:
        rounds += [tuple(r if k == odd else 0 for k in range(pointers)) for odd in range(pointers)]
    return rounds + [(8,) * pointers, (1,) * pointers]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bc1", "bc2", "bc3"])
def test_all_modes_at_misaligned_pointers(norm, n23, oracle, dev, fmt):
    """The input and each of the 3 (BC3: 12) outputs as the one misaligned pointer, which alone takes the call off the vector
    path; guard bytes around every output; BC1 also returns the flag."""
    outputs = 12 if fmt == "bc3" else 3
    rounds = pointer_rounds(1 + outputs, (1, 4, 8) if fmt == "bc3" else (4, 8, 1, 2))
    ins, outs, calls = Slots(0), Slots(0xA5), []
    for n in ALL_MODES_COUNTS:
        x = blocks_of(oracle, fmt, n)
        if fmt == "bc1":
            want, want_any = oracle.normalize_bc1_blocks_all_modes(x)
        else:
            want, want_any = (oracle.normalize_bc2_blocks_all_modes(x) if fmt == "bc2" else oracle.normalize_bc3_blocks_all_modes(x)), None
        assert n < 64 or len({w.tobytes() for w in want}) == outputs      # the outputs differ pairwise: none can stand in for another
        in_at = {}
        for rs in rounds:
            if rs[0] not in in_at:
                in_at[rs[0]] = ins.add(rs[0], f"{fmt} all-modes input n={n} at {rs[0]}", initial=x)
            calls.append((in_at[rs[0]], [outs.add(r, f"{fmt} all-modes n={n} pointers at {rs}: output {m}", nbytes=x.size, want=want[m])
                                         for m, r in enumerate(rs[1:])], want_any, (n, rs)))
    ins.upload(dev)
    outs.upload(dev)
    for i, ks, want_any, tag in calls:
        if fmt == "bc1":
            assert norm.normalize_blocks_all_modes(ins.view(i), [outs.view(k) for k in ks]) == want_any, tag
        else:
            n23.normalize_blocks_all_modes(fmt, ins.view(i), [outs.view(k) for k in ks])
    outs.check()
    ins.check()


# ------------------------------------------------------------------------------------------------------------
# 4. the change flag at single blocks
# ------------------------------------------------------------------------------------------------------------
def plain_blocks(oracle, n, seed):
    """n random BC1 blocks none of which any mode changes, as the CPU statement confirms; a block it would change gets indices the
    statement keeps (all four values in every row)"""
    x = oracle.fill_splitmix64(n * 8, seed)
    b = x.reshape(-1, 8)
    b[(oracle.normalize_bc1_blocks(x, COLOR0).reshape(-1, 8) != b).any(axis=1) |
      (oracle.normalize_bc1_blocks(x, REPL).reshape(-1, 8) != b).any(axis=1), 4:] = 0x1B
    outs, any_n = oracle.normalize_bc1_blocks_all_modes(x)
    assert not any_n and all(np.array_equal(o, x) for o in outs)
    return x


def plant(oracle, plain, at, kind):
    """a copy of `plain` whose block `at` alone is normalisable: solid (all pixels colour 0, which mode 1 rewrites) or fully
    transparent.  Returns (blocks, the three outputs of the CPU statement)."""
    x = plain.copy()
    b = x.reshape(-1, 8)
    if kind == "solid":
        b[at, 2:4] = b[at, 0:2] ^ 0x81          # c1 != c0 (mode 2 changes the block), and below: c1 != 0 (mode 1 does)
        b[at, 4:] = 0
        assert b[at, 2] or b[at, 3]
    else:
        b[at, 0:2] = 0                          # c0 = 0 <= c1, every pixel index 3
        b[at, 4:] = 0xFF
    outs, any_n = oracle.normalize_bc1_blocks_all_modes(x)
    others = np.arange(plain.size // 8) != at
    assert any_n
    for m, o in enumerate(outs):
        o = o.reshape(-1, 8)
        assert np.array_equal(o[others], b[others]) and ((o[at] != b[at]).any() or (m == 0 and kind == "solid")), (at, kind, m)
    return x, outs


def flag_positions(n):
    return sorted({p for p in (0, 1, 63, 64, 126, 127, 128, n - 2, n - 1) if 0 <= p < n})


@pytest.mark.gpu
def test_change_flag_at_single_blocks(norm, oracle, dev):
    """normalize_blocks_all_modes on plain blocks with one planted block: at residue 0 lanes take pairs and the odd last block a
    lane of its own, at residue 4 every block has its own lane.  True with the oracle's outputs; False, and three copies of the
    input, with nothing planted."""
    ins, outs, calls = Slots(0), Slots(0xA5), []
    for n in FLAG_COUNTS:
        plain = plain_blocks(oracle, n, 0xF1A6 + n)
        inputs = [(plain, [plain] * 3, False, "nothing planted")]
        for kind in ("solid", "transparent"):
            for at in flag_positions(n):
                x, want = plant(oracle, plain, at, kind)
                inputs.append((x, want, True, f"{kind} block at {at}"))
        for x, want, flag, what in inputs:
            for r in (0, 4):
                tag = f"flag n={n} {what} input at {r}"
                calls.append((ins.add(r, tag, initial=x), [outs.add(0, f"{tag}: output {m}", nbytes=x.size, want=want[m]) for m in range(3)],
                              flag, tag))
    ins.upload(dev)
    outs.upload(dev)
    for i, ks, flag, tag in calls:
        assert norm.normalize_blocks_all_modes(ins.view(i), [outs.view(k) for k in ks]) is flag, tag
    outs.check()
    ins.check()


@pytest.mark.gpu
@pytest.mark.parametrize("use_all", [False, True])
def test_auto_with_normalization_sees_one_block(pkg, oracle, use_all):
    """dxtlt_transform_bc1_auto_with_normalization, the only route to any_normalizable_kernel and to the fused mode 3: 20 001 plain
    blocks with one solid block at the odd last index, at index 0, and nowhere.  A missed flag gives no error, only a call log of
    4 | 8 entries where 3 x (4 | 8) are due."""
    from tests import cabi

    f = pkg.load().dxtlt_transform_bc1_auto_with_normalization
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(cabi.DltSizeEstimator), C.c_bool,
                  C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_bool), C.POINTER(C.c_uint32)]
    f.restype = C.c_int32
    plain = plain_blocks(oracle, 20_001, 0xA070)
    per_round = 8 if use_all else 4
    for at in (20_000, 0, None):
        x = plain if at is None else plant(oracle, plain, at, "solid")[0]
        log = []
        est, py_est = cabi.make_estimator("zlib", log)
        y = np.zeros_like(x)
        m, v, s, err = C.c_uint8(9), C.c_uint8(9), C.c_bool(False), C.c_uint32(0)
        rc = f(x.ctypes.data, y.ctypes.data, x.size, C.byref(est), use_all, C.byref(m), C.byref(v), C.byref(s), C.byref(err))
        assert rc == 0 and err.value == 0, (at, rc, err.value)
        want_choice, want_out, want_calls = oracle_auto.transform_bc1_auto_with_normalization(x, lambda b: py_est(bytes(b)), use_all)
        assert len(log) == (per_round if at is None else 3 * per_round), (at, len(log))
        assert log == (want_calls if at is not None else [ln for _off, ln in want_calls]), at
        assert (m.value, v.value, int(s.value)) == tuple(int(c) for c in want_choice), (at, want_choice)
        assert np.array_equal(y, want_out), at
