"""The case table, route model and runner of tests/test_host_paths_matrix.py.

Every format family reaches a device from host memory through host_round_trip (csrc/host_staging.cpp: mapped pinned pair,
one upload + launch + download, or the chunked pipeline) and run_sharded (csrc/host_sharded.cpp: per shard the pipeline or
one-shot slice copies), and every per-stream copy there is computed from a StreamLayout.  This module lists every distinct
layout the library can build, the unit counts that cross every chunk and shard boundary with a 64 KiB chunk, and what
dxtlt_debug_host_route_counts must report for each case under each environment -- worked out here from the documented
rules alone, so that a case which silently takes another arm, or a chunk rule that changes, fails.

Units are blocks (BC1-BC7) or pixels.  The first half of the module needs no device and no library."""
import collections
import time

import numpy as np

CHUNK_BYTES = 65536   # the smallest chunk DXTLT_PIPELINE_CHUNK_BYTES accepts (the override is masked with ~0xFFFF)
MIB = 1 << 20

ENVIRONMENTS = {
    # whole buffers and shards of 64 KiB or more go through upload | kernel | download in 64 KiB chunks
    "pipeline": {"DXTLT_MAPPED_MAX_BYTES": "1", "DXTLT_PIPELINE_MIN_BYTES": str(CHUNK_BYTES),
                 "DXTLT_PIPELINE_CHUNK_BYTES": str(CHUNK_BYTES)},
    # mapped staging off: buffers take one upload + launch + download, shards the per-slice copies
    "one_shot": {"DXTLT_MAPPED_MAX_BYTES": "1"},
    # the shipped thresholds: everything here is below 1 MiB, so buffers take the mapped pair
    "default": {},
}
# (largest buffer of the mapped pair, smallest buffer or shard of the pipeline) in bytes, as each environment sets them
THRESHOLDS = {"pipeline": (1, CHUNK_BYTES), "one_shot": (1, 96 * MIB), "default": (MIB, 96 * MIB)}

MAPPED, ONE_SHOT, PIPELINED, CHUNKS, SHARD_ONE_SHOT = range(5)   # dxtlt_debug_host_route_counts

GRANULE = 1024
INTERLEAVED, PLANAR, PLANAR_DELTA = 0, 1, 2

# family: "block" (BC1-BC5, dxtlt_transform_sharded), "granule" (BC6H / BC7: a tail part behind the streams, sharded calls of
# their own), "pixel" (format codes 8 / 9), "normalize" (BC1 forward with fused block normalisation: host call only).
# settings: bc1 / bc2 (variant, split colour); bc3 (variant, split alpha, split colour); bc4 / bc5 (split endpoints,);
# pixels (decorrelate, layout); normalize (color mode, variant, split colour).
# unit: bytes per block / pixel; align: a chunk and a shard start on a multiple of it; shard_unit: at most one shard per so many.
Layout = collections.namedtuple("Layout", "name family fmt settings unit align shard_unit")
Case = collections.namedtuple("Case", "layout path units shards")   # path "host" (shards 0) or "sharded"


def layouts():
    out = []

    def block(fmt, unit, *settings):
        out.append(Layout(f"{fmt}{list(settings)}", "block", fmt, settings, unit, 2048, 1))

    block("bc1", 8, 1, False)
    block("bc1", 8, 2, True)
    block("bc2", 16, 1, False)
    block("bc2", 16, 3, True)
    for variant, (sa, sc) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        block("bc3", 16, variant, sa, sc)
    for fmt, unit in (("bc4", 8), ("bc5", 16)):
        for split in (False, True):
            block(fmt, unit, split)
    for fmt in ("bc6h", "bc7"):
        out.append(Layout(fmt, "granule", fmt, (), 16, GRANULE, GRANULE))
    for B in (3, 4):
        for settings in ((True, INTERLEAVED), (True, PLANAR), (True, PLANAR_DELTA), (False, PLANAR_DELTA)):
            out.append(Layout(f"pixels{B}{list(settings)}", "pixel", f"pixels{B}", settings, B, 4096, 4096))
    for color_mode, variant in ((1, 1), (2, 3)):
        out.append(Layout(f"bc1+normalize{[color_mode, variant, True]}", "normalize", "bc1", (color_mode, variant, True), 8, 2048, 1))
    return out


def chunk_units(layout):
    """The pipeline's chunk in units under CHUNK_BYTES: floor(bytes / unit) rounded down to a multiple of the alignment.  3-byte
    pixels do not divide a power of two: 21 845 pixels round down to 20 480."""
    c = CHUNK_BYTES // layout.unit
    return c - c % layout.align


def host_sizes(layout):
    C, A = chunk_units(layout), layout.align
    if layout.family == "granule":
        # whole granules of three full chunks / of one chunk and a rest, each with a tail part of 0, 1 and 1023 blocks
        return [main + tail for main in (3 * C, C + GRANULE) for tail in (0, 1, GRANULE - 1)]
    # the last chunk full; a rest of one unit; one chunk and one unit; a rest one unit short of an alignment step
    return [3 * C, 3 * C + 1, C + 1, 2 * C + A - 1]


def sharded_sizes(layout):
    """(shards asked for, units)"""
    C, A = chunk_units(layout), layout.align
    return [(3, 3 * (2 * C + A) + 5),   # every shard two chunks and a rest at a non-zero base, the last one ragged
            (3, 2 * A + 3),             # the share rounds down to 0: two empty shards, the last holds everything
            (64, 5 * A + 1)]            # capped by the shard unit (granules, pixels) or mostly empty (blocks)


def cases_of(layout):
    host = [Case(layout, "host", n, 0) for n in host_sizes(layout)]
    if layout.family == "normalize":     # dxtlt_transform_sharded has no normalising form
        return host
    return host + [Case(layout, "sharded", n, shards) for shards, n in sharded_sizes(layout)]


def ordered_cases():
    """Every case once: round k takes case k of every layout, the layouts in an order that alternates the families and every
    second layout starting one case later -- so consecutive calls differ in family and mostly in size, and the thread's
    grow-only staging, the mapped pair and the shard context pool are reused, regrown and reused across formats."""
    by_family = collections.defaultdict(list)
    for L in layouts():
        by_family[L.family].append(L)
    queues = [by_family[f] for f in ("block", "pixel", "granule", "normalize")]
    order = []
    while any(queues):
        for q in queues:
            if q:
                order.append(q.pop(0))
    out = []
    rounds = max(len(cases_of(L)) for L in order)
    for k in range(rounds):
        for j, L in enumerate(order):
            mine = cases_of(L)
            if k < len(mine):
                out.append(mine[(k + j) % len(mine)])
    assert len(out) == len(set(out)) == sum(len(cases_of(L)) for L in order)
    return out


def case_count():
    return sum(len(cases_of(L)) for L in layouts())


def case_name(case):
    return f"{case.layout.name} {case.path} {case.units}" + (f" in {case.shards} shards" if case.shards else "")


# ---- the route model ------------------------------------------------------------------------------------------------------------
def plan_shards(layout, units, shards_asked):
    """[(first, count)]: at most 64 shards and one per shard unit; equal shares rounded down to the alignment, the last shard
    takes the rest"""
    shards = min(shards_asked, 64, -(-units // layout.shard_unit))
    share = units // shards
    share -= share % layout.align
    return [(i * share, units - i * share if i == shards - 1 else share) for i in range(shards)]


def _round_trip(env, layout, units, counts):
    mapped_max, pipeline_min = THRESHOLDS[env]
    nbytes = units * layout.unit
    if nbytes <= mapped_max:
        counts[MAPPED] += 1
    elif nbytes >= pipeline_min:
        counts[PIPELINED] += 1
        counts[CHUNKS] += -(-units // chunk_units(layout))
    else:
        counts[ONE_SHOT] += 1


def expected_counts(env, case):
    """What ONE call of the case (either direction) adds to the five counters"""
    L, n = case.layout, case.units
    pipeline_min = THRESHOLDS[env][1]
    counts = [0] * 5
    tail = n % GRANULE if L.family == "granule" else 0
    main = n - tail
    if case.path == "host":
        if tail and main and n * L.unit >= pipeline_min:
            # the pipeline moves stream slices: whole granules first, then the tail part as the buffer of its own that it is
            _round_trip(env, L, main, counts)
            _round_trip(env, L, tail, counts)
        else:
            _round_trip(env, L, n, counts)
        return counts
    for first, count in plan_shards(L, n, case.shards):
        if count == 0:
            continue
        in_main = max(0, min(first + count, main) - first)
        if in_main and in_main * L.unit >= pipeline_min:
            counts[PIPELINED] += 1
            counts[CHUNKS] += -(-in_main // chunk_units(L))
            if count > in_main:
                counts[SHARD_ONE_SHOT] += 1   # the tail part the last shard holds
        else:
            counts[SHARD_ONE_SHOT] += 1
    return counts


def stream_table(layout, pkg=None, granule_streams=None):
    """The StreamLayout of a layout as ((offset multiplier, width), ...): formats 1-5 from the package's own table, pixels as
    docs/PIXEL_FORMAT.md has them (one stream of whole pixels, or a plane of one byte per pixel at c * P), the granule formats
    as the caller passes them in."""
    if layout.family == "pixel":
        B = layout.unit
        return ((0, B),) if layout.settings[1] == INTERLEAVED else tuple((c, 1) for c in range(B))
    if layout.family == "granule":
        return tuple(granule_streams)
    return tuple(pkg.stream_table(layout.fmt, block_settings(pkg, layout)))


def block_settings(pkg, layout):
    fmt, s = layout.fmt, layout.settings
    if layout.family == "normalize":
        return pkg.Bc1TransformSettings(pkg.YCoCgVariant(s[1]), s[2])
    if fmt in ("bc4", "bc5"):
        return getattr(pkg, f"Bc{fmt[2]}TransformSettings")(s[0])
    return getattr(pkg, f"Bc{fmt[2]}TransformSettings")(pkg.YCoCgVariant(s[0]), *s[1:])


# ---- the runner (child process: needs the library and a device) -----------------------------------------------------------------
GUARD = 64


class Guarded:
    """a host output of n bytes filled with 0xEE between two guards of 64 bytes of 0xA5"""

    def __init__(self, n):
        self.whole = np.full(n + 2 * GUARD, 0xA5, dtype=np.uint8)
        self.out = self.whole[GUARD:GUARD + n]
        self.out[:] = 0xEE

    def guards_intact(self):
        return bool((self.whole[:GUARD] == 0xA5).all() and (self.whole[GUARD + self.out.size:] == 0xA5).all())


class Runner:
    def __init__(self, env, pkg, oracle):
        import bc45_ref
        import bc6h_ref
        import pixels_ref
        from dxt_lossless_transform_amd import bc6h, bc7, normalize, pixels
        from tests.test_bc6h_gpu import blocks_of
        from tests.test_bc7 import make_blocks
        from tests.test_normalize import crafted_blocks

        self.env, self.pkg, self.oracle = env, pkg, oracle
        self.bc45_ref, self.bc6h_ref, self.pixels_ref = bc45_ref, bc6h_ref, pixels_ref
        self.granule_mod = {"bc6h": bc6h, "bc7": bc7}
        self.normalize, self.pixels = normalize, pixels
        self.bc6h_blocks, self.bc7_blocks, self.crafted_blocks = blocks_of, make_blocks, crafted_blocks

    # (input, the CPU statement's transform of it)
    def data(self, case):
        L, n = case.layout, case.units
        seed = n * 31 + len(L.name)
        if L.family == "granule":
            if L.fmt == "bc6h":
                x = self.bc6h_blocks(n, "uniform", seed)
                return x, self.bc6h_ref.transform(x)
            x = self.bc7_blocks(self.oracle, n, "uniform", seed)
            return x, self.oracle.transform_bc7(x)
        if L.family == "normalize":
            x = self.crafted_blocks(self.oracle, n, seed)
            want = self.oracle.transform_bc1_with_normalize_blocks(x, *L.settings)
            assert not np.array_equal(want, self.oracle.transform("bc1", x, L.settings[1], L.settings[2])), "nothing to normalise"
            return x, want
        x = np.random.default_rng(seed).integers(0, 256, n * L.unit, dtype=np.uint8)
        if L.family == "pixel":
            want = self.pixels_ref.forward(x, L.unit, *L.settings)
            assert np.array_equal(self.pixels_ref.inverse(want, L.unit, *L.settings), x)
            return x, want
        if L.fmt in ("bc4", "bc5"):
            want = self.bc45_ref.transform(L.fmt, x, L.settings[0])
            assert np.array_equal(self.bc45_ref.untransform(L.fmt, want, L.settings[0]), x)
            return x, want
        if L.fmt == "bc3":
            variant, sa, sc = L.settings
            return x, self.oracle.transform("bc3", x, variant, sc, sa)
        return x, self.oracle.transform(L.fmt, x, L.settings[0], L.settings[1])

    def call(self, case, inverse, src, dst):
        L, pkg = case.layout, self.pkg
        if L.family == "normalize":
            assert not inverse
            return self.normalize.transform_bc1_with_normalize_blocks(
                src, dst, self.normalize.Bc1TransformDetailsWithNormalization(self.normalize.ColorNormalizationMode(L.settings[0]),
                                                                              L.settings[1], L.settings[2]))
        if L.family == "granule":
            mod = self.granule_mod[L.fmt]
            if case.path == "host":
                return getattr(mod, f"{'un' if inverse else ''}transform_{L.fmt}")(src, dst)
            return getattr(mod, f"transform_{L.fmt}_sharded")(src, dst, case.shards, inverse=inverse)
        if L.family == "pixel":
            if case.path == "host":
                return (self.pixels.untransform_pixels if inverse else self.pixels.transform_pixels)(src, dst, L.unit, *L.settings)
            return self.pixels.transform_pixels_sharded(src, dst, L.unit, *L.settings, num_shards=case.shards, inverse=inverse)
        st = block_settings(pkg, L)
        if case.path == "host":
            return getattr(pkg, f"{'un' if inverse else ''}transform_{L.fmt}_with_settings")(src, dst, st)
        return pkg.transform_sharded(L.fmt, inverse, src, dst, st, case.shards)

    def check_direction(self, case, inverse, src, want):
        name = "inverse" if inverse else "forward"
        kept, g = src.copy(), Guarded(src.size)
        before = self.pkg.host_route_counts()
        self.call(case, inverse, src, g.out)
        after = self.pkg.host_route_counts()
        assert g.guards_intact(), (name, "guard bytes around the output were written")
        assert np.array_equal(src, kept), (name, "the input was written")
        if not np.array_equal(g.out, want):
            at = int(np.flatnonzero(g.out != want)[0])
            raise AssertionError((name, f"differs from the CPU statement from byte {at} of {want.size}",
                                  "never written" if g.out[at] == 0xEE else "wrong value"))
        delta = [a - b for a, b in zip(after, before)]
        assert delta == expected_counts(self.env, case), (name, "routes taken", delta, "expected", expected_counts(self.env, case))
        if case.path == "sharded" and case.layout.family != "granule":
            # dxtlt_sharded_last_stats (formats 1-5, 8, 9): the shards tile [0, units) in order, all but the last on the alignment
            stats = self.pkg.sharded_last_stats()
            got = [(s["first_block"], s["blocks"]) for s in stats]
            assert got == plan_shards(case.layout, case.units, case.shards), (name, "shard ranges", got)
            at = 0
            for first, count in got:
                assert first == at, (name, "shard ranges do not tile the array", got)
                at += count
            assert at == case.units and all(count % case.layout.align == 0 for _, count in got[:-1]), (name, got)

    def check(self, case):
        x, want = self.data(case)
        self.check_direction(case, False, x, want)
        if case.layout.family != "normalize":
            # the inverse of the CPU statement's forward output, not of the device's
            self.check_direction(case, True, want, x)


def run_all(env, pkg, oracle):
    """The child process.  Failures are collected so that one run names every failing case; a device error (anything but a
    refused argument) ends the run at once."""
    runner = Runner(env, pkg, oracle)
    todo = ordered_cases()
    failures, passed, t0 = [], 0, time.perf_counter()
    for k, case in enumerate(todo):
        if k == len(todo) // 2:
            pkg.load().dxtlt_release_thread_resources()   # once, mid-run: everything after it allocates afresh
        try:
            runner.check(case)
            passed += 1
        except AssertionError as e:
            failures.append(f"FAILED {case_name(case)}: {e.args[0] if e.args else e}")
        except pkg.DeviceError as e:
            failures.append(f"FAILED {case_name(case)}: {e}")
            if e.code not in (1, 2):
                break
    for line in failures:
        print(line)
    print(f"{env}: checked {passed} (layout, size, path) cases of {len(todo)}, forward and inverse, "
          f"in {time.perf_counter() - t0:.1f} s")
    return 1 if failures else 0
