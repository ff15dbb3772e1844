"""The selection step of the auto transforms with a scripted estimator: every candidate wins, ties, the all-maximum estimator and
a failing estimate at every call, on every route of dxtlt_transform_{bc1..bc5}_auto; the host-side pick of the device routes
without a device (dxtlt_debug_auto_pick).

The expected choice and bytes always come from the CPU statements (oracle/oracle_auto.py, tests/bc45_ref.py) run with the same
table of answers, never from the library.  A table is keyed by a section's (len, crc32): the inputs are seeded random blocks whose
distinct sections have pairwise different keys, which is asserted on the CPU before any device call (N = 1 cannot satisfy it: split
equals no split there).  N = 129 makes the staged slot rounding (2N + 255) & ~255 non-trivial, N = 4099 is odd and spans several
workgroups."""
import contextlib
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import bc45_ref
import cabi
from oracle import oracle_auto, oracle_c

FMT_ID = {"bc1": 1, "bc2": 2, "bc3": 3, "bc4": 4, "bc5": 5}
BLOCK = {"bc1": 8, "bc2": 16, "bc3": 16, "bc4": 8, "bc5": 16}
KINDS = [(f, u) for f in ("bc1", "bc2", "bc3") for u in (False, True)] + [("bc4", False), ("bc5", False)]
KINDS_123 = [k for k in KINDS if k[0] in ("bc1", "bc2", "bc3")]
SIZES = (129, 4099)
SIZE_MAX = cabi.SIZE_MAX
E_ESTIMATOR = 5                       # DXTLT_E_ESTIMATOR
# Bc1/Bc2TransformSettings::default() = {Variant1, split}; Bc3 = {Variant1, split alphas, split colours}; BC4 / BC5: no split.
# Under the all-maximum tables: for BC1 / BC2 the default is also the LAST candidate of both reference orders, so they tell "the
# default was kept" from "the first total was taken" but not from "the last candidate was taken" (`<=`); for BC4 / BC5 the default
# is the FIRST candidate, so they tell it from `<=` but not from a search started at the first total; BC3's default is neither
# first nor last of its orders and pins both.
DEFAULTS = {"bc1": (1, 0, 1), "bc2": (1, 0, 1), "bc3": (1, 1, 1), "bc4": (0, 0, 0), "bc5": (0, 0, 0)}
ROUTES = ("staged", "no_arena", "threads4")      # (a) arena + staged downloads, one thread; (b) one full transform per candidate; (c)
SEQUENTIAL = ("staged", "no_arena")


# ---- inputs and tables ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(fmt, blocks, use_all):
    """(x, candidate_sections, {section id: key}) of seeded random blocks; the key condition is asserted here, on the CPU"""
    oracle_c.lib()
    x = np.random.default_rng(0xA070_0000 + 16 * blocks + FMT_ID[fmt]).integers(0, 256, blocks * BLOCK[fmt], dtype=np.uint8)
    secs = cabi.candidate_sections(fmt, x, use_all)
    keys = cabi.distinct_sections(secs)
    x.setflags(write=False)
    return x, secs, keys


@functools.lru_cache(maxsize=None)
def norm_case(blocks, use_all):
    """crafted_blocks of tests/test_normalize.py and its 3 x 4 / 3 x 8 colour sections, pairwise different"""
    from test_normalize import crafted_blocks

    oracle_c.lib()
    x = crafted_blocks(oracle_c, blocks, blocks + 7)
    secs = cabi.normalization_sections(x, use_all)
    assert len(secs) == 3 * (8 if use_all else 4) and len({key for _c, key in secs}) == len(secs)
    x.setflags(write=False)
    return x, secs


def winner_table(secs, keys, k):
    """candidate k the unique minimum: its section(s) 10, every other section 20 (BC3: k's total is 20, a candidate that shares one
    section with it has 30, the others 40)"""
    table = {key: 20 for key in keys.values()}
    for _sid, key in secs[k][1]:
        table[key] = 10
    return table


def tie_tables(fmt, secs, keys):
    """[(name, table, default)]: all sizes equal; BC1 / BC2 every pair of candidates at the minimum together; BC3 both alpha sections
    equal and every pair of colour sections at the minimum; BC5 the two candidates level through crossed halves"""
    tables = [("all equal", {}, 7)]
    if fmt in ("bc1", "bc2"):
        for i, j in itertools.combinations(range(len(secs)), 2):
            t = {key: 20 for key in keys.values()}
            t[secs[i][1][0][1]] = t[secs[j][1][0][1]] = 10
            tables.append((f"pair {i} {j}", t, None))
    if fmt == "bc3":
        colours = sorted(sid for sid in keys if sid[0] == "c")
        for a, b in itertools.combinations(colours, 2):
            t = {keys[sid]: 20 for sid in colours}
            t[keys[a]] = t[keys[b]] = 10
            t[keys[("a", 0)]] = t[keys[("a", 1)]] = 5
            tables.append((f"colours {a} {b}", t, None))
    if fmt == "bc5":
        tables.append(("crossed", {keys[("r", 0)]: 10, keys[("g", 0)]: 20, keys[("r", 1)]: 20, keys[("g", 1)]: 10}, None))
    return tables


def maximum_table(fmt, keys):
    """every section answers SIZE_MAX; BC3: alpha 0, colour SIZE_MAX, which keeps the sum from wrapping"""
    return ({keys[("a", 0)]: 0, keys[("a", 1)]: 0} if fmt == "bc3" else {}), SIZE_MAX


def cpu_auto(fmt, x, use_all, table, default, fail_at=None):
    """the CPU statement with the scripted answers: (choice, output, log, None), or (None, None, log, code) where an estimate fails"""
    log = []
    est = cabi.scripted_estimate(table, default, log, fail_at)
    try:
        if fmt in ("bc4", "bc5"):
            split = bc45_ref.auto_choice(fmt, x, est)
            return (0, int(split), 0), bc45_ref.transform(fmt, x, split), log, None
        choice, out, _calls = oracle_auto.transform_auto(fmt, x, est, use_all)
        return tuple(int(c) for c in choice), out, log, None
    except cabi.ScriptedFailure as f:
        return None, None, log, f.code


# ---------------------------------------------------------------------------------------------------------------
# CPU: the statements themselves
# ---------------------------------------------------------------------------------------------------------------
def test_orders_are_the_references_lists():
    """(YCoCgVariant, split colours) of bc1 / bc2 and (YCoCgVariant, split alphas, split colours) of bc3, core numbering None 0,
    Variant1..3 1..3, as read from the reference's settings.rs"""
    # dxt-lossless-transform-bc1/src/transform/settings.rs:81-86 (bc2 settings.rs:81-86 is the same list)
    fast_12 = [(0, False), (0, True), (1, False), (1, True)]
    # dxt-lossless-transform-bc1/src/transform/settings.rs:89-98 (bc2 settings.rs:89-98)
    all_12 = [(2, False), (0, False), (0, True), (3, False), (3, True), (2, True), (1, False), (1, True)]
    # dxt-lossless-transform-bc3/src/transform/settings.rs:91-100
    fast_3 = [(1, True, False), (1, True, True), (0, True, False), (0, False, True), (0, True, True), (1, False, True),
              (0, False, False), (1, False, False)]
    # dxt-lossless-transform-bc3/src/transform/settings.rs:104-121
    all_3 = [(2, True, False), (2, True, True), (3, True, True), (3, True, False), (1, True, False), (3, False, True),
             (1, True, True), (2, False, True), (2, False, False), (3, False, False), (0, True, False), (0, False, True),
             (0, True, True), (1, False, True), (0, False, False), (1, False, False)]
    for fmt in ("bc1", "bc2"):
        assert oracle_auto.test_order(fmt, False) == [(v, 0, int(sc)) for v, sc in fast_12]
        assert oracle_auto.test_order(fmt, True) == [(v, 0, int(sc)) for v, sc in all_12]
    assert oracle_auto.test_order("bc3", False) == [(v, int(sa), int(sc)) for v, sa, sc in fast_3]
    assert oracle_auto.test_order("bc3", True) == [(v, int(sa), int(sc)) for v, sa, sc in all_3]
    for order in (fast_12, all_12, fast_3, all_3):
        assert len(set(order)) == len(order)
    assert set(all_3) == {(v, sa, sc) for v in range(4) for sa in (False, True) for sc in (False, True)}


@pytest.mark.parametrize("fmt,use_all", KINDS)
def test_statements_keep_the_defaults_under_the_maximum_and_the_first_under_ties(fmt, use_all):
    x, secs, keys = case(fmt, 129, use_all)
    table, default = maximum_table(fmt, keys)
    choice, out, log, code = cpu_auto(fmt, x, use_all, table, default)
    assert code is None and choice == DEFAULTS[fmt]
    assert np.array_equal(out, cabi.cpu_transform(fmt, x, DEFAULTS[fmt]))
    assert log == [key for _c, ss in secs for _sid, key in ss]                # every candidate was still tried, in order
    choice, out, _log, code = cpu_auto(fmt, x, use_all, {}, 7)
    assert code is None and choice == secs[0][0] and np.array_equal(out, cabi.cpu_transform(fmt, x, secs[0][0]))
    # one below the maximum is a size like any other: the first candidate that answers it wins
    if len(secs[1][1]) == 1:
        assert cpu_auto(fmt, x, use_all, {secs[1][1][0][1]: SIZE_MAX - 1}, SIZE_MAX)[0] == secs[1][0]
    for k in range(len(secs)):
        assert cpu_auto(fmt, x, use_all, winner_table(secs, keys, k), None)[0] == secs[k][0]


@pytest.mark.parametrize("use_all", [False, True])
def test_normalization_statement_keeps_the_defaults_under_the_maximum_and_the_first_under_ties(use_all):
    x, secs = norm_case(129, use_all)
    run = oracle_auto.transform_bc1_auto_with_normalization
    choice, out, calls = run(x, cabi.scripted_estimate({}, SIZE_MAX), use_all)
    assert tuple(choice) == (0, 1, 1) and len(calls) == len(secs)
    assert np.array_equal(out, oracle_c.transform("bc1", x, 1, True))
    choice, _out, _calls = run(x, cabi.scripted_estimate({}, 7), use_all)
    assert tuple(choice) == secs[0][0]
    choice, _out, _calls = run(x, cabi.scripted_estimate({}, ("fail", 3)), use_all)
    assert tuple(choice) == (0, 1, 1)


# ---------------------------------------------------------------------------------------------------------------
# CPU: the host-side pick of the device routes (dxtlt_debug_auto_pick), no device
# ---------------------------------------------------------------------------------------------------------------
PICK_ROUTES = (0, 1, 2)       # single-buffer device route, batch route, single-buffer route without its arena
JUNK = 1 << 50                # in a slot the route never reads


@pytest.fixture(scope="module")
def picker(pkg):
    l = C.CDLL(pkg._lib.lib_path())
    u64p, bp = C.POINTER(C.c_uint64), C.POINTER(C.c_bool)
    l.dxtlt_debug_auto_pick.argtypes = [C.c_int32, C.c_int32, C.c_bool, u64p, C.c_int32, u64p, C.c_int32, C.POINTER(C.c_uint8), bp, bp]
    l.dxtlt_debug_auto_pick.restype = C.c_int32

    def pick(route, fmt, use_all, vec, cap=16):
        arr = (C.c_uint64 * len(vec))(*vec)
        totals = (C.c_uint64 * 16)(*([0xDEAD] * 16))
        mode, sa, sc = C.c_uint8(0xEE), C.c_bool(False), C.c_bool(False)
        rc = l.dxtlt_debug_auto_pick(route, FMT_ID[fmt], use_all, arr, len(vec), totals, cap, C.byref(mode), C.byref(sa), C.byref(sc))
        return rc, (mode.value, int(sa.value), int(sc.value)), list(totals)

    return pick


def section_ids(fmt, cand):
    mode, sa, sc = cand
    return {"bc1": [("c", mode, sc)], "bc2": [("c", mode, sc)], "bc3": [("a", sa), ("c", mode, sc)], "bc4": [("e", sa)],
            "bc5": [("r", sa), ("g", sa)]}[fmt]


def size_vector(route, fmt, use_all, sizes):
    """{section id: size} in the order the route's counters come back (include/dxtlt_estimator.h, dxtlt_debug_auto_pick)"""
    cands = cabi.auto_candidates(fmt, use_all)
    if route == 2 or (route == 0 and fmt in ("bc4", "bc5")):                   # two slots per candidate
        vec = []
        for cand in cands:
            ids = section_ids(fmt, cand)
            vec += [sizes[i] for i in ids] + [JUNK] * (2 - len(ids))
        return vec
    colours = [sizes[("c", v, sc)] for v in range(4 if use_all else 2) for sc in (0, 1)] if fmt in ("bc1", "bc2", "bc3") else []
    alphas = [sizes[("a", 0)], sizes[("a", 1)]] if fmt == "bc3" else []
    if fmt == "bc4":
        return [sizes[("e", 0)], sizes[("e", 1)]]
    if fmt == "bc5":
        return [sizes[("r", 0)], sizes[("r", 1)], sizes[("g", 0)], sizes[("g", 1)]]
    return alphas + colours                                                  # the arena's and the batch slice's order: memory order


def check_pick(picker, fmt, use_all, sizes, what):
    cands = cabi.auto_candidates(fmt, use_all)
    totals = [sum(sizes[i] for i in section_ids(fmt, c)) for c in cands]
    want = cands[totals.index(min(totals))]                                     # the first minimum of the order
    for route in PICK_ROUTES:
        rc, got, got_totals = picker(route, fmt, use_all, size_vector(route, fmt, use_all, sizes))
        assert rc == 0, (what, route)
        assert got_totals[:len(cands)] == totals and got_totals[len(cands):] == [0xDEAD] * (16 - len(cands)), (what, route)
        assert got == want, (what, route, got, want)
    return want


@pytest.mark.parametrize("fmt,use_all", KINDS)
def test_pick_every_candidate_wins_ties_and_totals(picker, fmt, use_all):
    cands = cabi.auto_candidates(fmt, use_all)
    ids = sorted({i for c in cands for i in section_ids(fmt, c)})
    assert cands == ([(0, 0, 0), (0, 1, 0)] if fmt in ("bc4", "bc5") else oracle_auto.test_order(fmt, use_all))
    for k, cand in enumerate(cands):                                            # every candidate the unique winner
        sizes = {i: 20 for i in ids}
        sizes.update({i: 10 for i in section_ids(fmt, cand)})
        assert check_pick(picker, fmt, use_all, sizes, ("winner", k)) == cand
    rng = np.random.default_rng(0x91C4 + FMT_ID[fmt] * 2 + use_all)
    for rep in range(8):                                                        # every section its own size: the sums, index by index
        sizes = {i: int(v) for i, v in zip(ids, rng.permutation(1 << 16)[:len(ids)].astype(np.int64) + (rep << 40))}
        check_pick(picker, fmt, use_all, sizes, ("distinct", rep))
    assert check_pick(picker, fmt, use_all, {i: 7 for i in ids}, "all equal") == cands[0]
    if fmt in ("bc1", "bc2"):
        for i, j in itertools.combinations(range(len(cands)), 2):
            sizes = {s: 20 for s in ids}
            sizes[section_ids(fmt, cands[i])[0]] = sizes[section_ids(fmt, cands[j])[0]] = 10
            assert check_pick(picker, fmt, use_all, sizes, ("pair", i, j)) == cands[i]
    if fmt == "bc3":
        colours = [i for i in ids if i[0] == "c"]
        for a, b in itertools.combinations(colours, 2):
            sizes = {i: 20 for i in colours}
            sizes.update({a: 10, b: 10, ("a", 0): 5, ("a", 1): 5})
            want = check_pick(picker, fmt, use_all, sizes, ("colours", a, b))
            assert want == next(c for c in cands if ("c", c[0], c[2]) in (a, b))
    if fmt == "bc5":
        assert check_pick(picker, fmt, use_all, {("r", 0): 10, ("g", 0): 20, ("r", 1): 20, ("g", 1): 10}, "crossed") == cands[0]
    if fmt == "bc4":
        assert check_pick(picker, fmt, use_all, {("e", 0): 10, ("e", 1): 9}, "split") == (0, 1, 0)


def test_pick_refuses_what_no_route_reads_back(picker):
    assert picker(0, "bc3", True, [1] * 9)[0] == 2 and picker(1, "bc5", False, [1] * 2)[0] == 2       # DXTLT_E_INVALID_ARGUMENT
    assert picker(3, "bc1", False, [1] * 4)[0] == 2
    rc, got, totals = picker(1, "bc1", True, [9, 8, 7, 6, 5, 4, 3, 2], cap=3)                            # at most cap totals
    assert rc == 0 and got == (3, 0, 1) and totals[:4] == [5, 9, 8, 0xDEAD]


# ---------------------------------------------------------------------------------------------------------------
# GPU: dxtlt_transform_{bc1..bc5}_auto with the scripted estimator, on every route
# ---------------------------------------------------------------------------------------------------------------
CORE_S = {1: cabi.CoreSettings2, 2: cabi.CoreSettings2, 3: cabi.CoreSettings3}


@pytest.fixture(scope="module")
def lib(pkg):
    l = cabi.bind(C.CDLL(pkg._lib.lib_path()))
    vp, sz, b, i32 = C.c_void_p, C.c_size_t, C.c_bool, C.c_int32
    u8p, bp, estp, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_bool), C.POINTER(cabi.DltSizeEstimator), C.POINTER(C.c_uint32)
    for n in ("bc1", "bc2"):
        getattr(l, f"dxtlt_transform_{n}_auto").argtypes = [vp, vp, sz, estp, b, u8p, bp, u32p]
    l.dxtlt_transform_bc3_auto.argtypes = [vp, vp, sz, estp, b, u8p, bp, bp, u32p]
    for n in ("bc4", "bc5"):
        getattr(l, f"dxtlt_transform_{n}_auto").argtypes = [vp, vp, sz, estp, bp]
        getattr(l, f"dxtlt_untransform_{n}_with_settings").argtypes = [vp, vp, sz, b]
    l.dxtlt_transform_bc1_auto_with_normalization.argtypes = [vp, vp, sz, estp, b, u8p, u8p, bp, u32p]
    l.dxtlt_debug_auto_use_arena.argtypes, l.dxtlt_debug_auto_use_arena.restype = [i32], None
    l.dxtlt_debug_auto_last_estimator_error.argtypes, l.dxtlt_debug_auto_last_estimator_error.restype = [], C.c_uint32
    l.dxtlt_set_auto_estimator_threads.argtypes, l.dxtlt_set_auto_estimator_threads.restype = [i32], None
    l.dxtlt_last_error.restype = C.c_char_p
    return l


@contextlib.contextmanager
def on_route(lib, name):
    try:
        if name == "no_arena":
            lib.dxtlt_debug_auto_use_arena(0)
        if name == "threads4":
            lib.dxtlt_set_auto_estimator_threads(4)
        yield
    finally:
        lib.dxtlt_debug_auto_use_arena(1)
        lib.dxtlt_set_auto_estimator_threads(1)


def call_auto(lib, fmt, x, est, use_all, unlike=(0, 0, 0)):
    """(rc, reported settings, output, estimator error or None); the out parameters start unlike the settings `unlike`"""
    y = np.full(x.size, 0xEE, dtype=np.uint8)
    mode, err = C.c_uint8(unlike[0] ^ 0x80), C.c_uint32(0xEEEE)
    sa, sc = C.c_bool(not unlike[1]), C.c_bool(not unlike[2])
    f = getattr(lib, f"dxtlt_transform_{fmt}_auto")
    if fmt in ("bc4", "bc5"):
        rc = f(x.ctypes.data, y.ctypes.data, x.size, C.byref(est), C.byref(sa))
        return rc, (0, int(sa.value), 0), y, None
    if fmt == "bc3":
        rc = f(x.ctypes.data, y.ctypes.data, x.size, C.byref(est), use_all, C.byref(mode), C.byref(sa), C.byref(sc), C.byref(err))
        return rc, (mode.value, int(sa.value), int(sc.value)), y, err.value
    rc = f(x.ctypes.data, y.ctypes.data, x.size, C.byref(est), use_all, C.byref(mode), C.byref(sc), C.byref(err))
    return rc, (mode.value, 0, int(sc.value)), y, err.value


def core_settings(n, choice):
    st = CORE_S[n]()
    st.DecorrelationMode, st.SplitColourEndpoints = choice[0], bool(choice[2])
    if n == 3:
        st.SplitAlphaEndpoints = bool(choice[1])
    return st


def untransform(lib, fmt, y, choice):
    z = np.full(y.size, 0xDD, dtype=np.uint8)
    if fmt in ("bc4", "bc5"):
        rc = getattr(lib, f"dxtlt_untransform_{fmt}_with_settings")(y.ctypes.data, z.ctypes.data, y.size, bool(choice[1]))
    else:
        n = FMT_ID[fmt]
        rc = getattr(lib, f"dltbc{n}core_untransform")(y.ctypes.data, y.size, z.ctypes.data, z.size, core_settings(n, choice)).ErrorCode
    assert rc == 0
    return z


def check_exact(lib, fmt, blocks, use_all, table, default, route, what, max_extra=64, want_choice=None):
    """one succeeding call on `route`: rc 0, the CPU statement's choice, its bytes, its sequence of sections; the inverse call with
    the reported settings returns the input"""
    x, _secs, keys = case(fmt, blocks, use_all)
    choice, out, cpu_log, code = cpu_auto(fmt, x, use_all, table, default)
    assert code is None and (want_choice is None or choice == want_choice), (what, choice, want_choice)
    log = []
    est = cabi.scripted_estimator(table, default, log, max_extra=max_extra)
    with on_route(lib, route):
        rc, got, y, err = call_auto(lib, fmt, x, est, use_all, unlike=choice)
    assert rc == 0 and err in (0, None), (what, route, rc, err, lib.dxtlt_last_error())
    # (set by the five dxtlt_transform_bcN_auto entry points alone: it says nothing after the core calls, the stable builder or
    # the normalisation route, which leave the thread's earlier value)
    assert lib.dxtlt_debug_auto_last_estimator_error() == 0, (what, route)
    assert got == choice, (what, route, got, choice)
    assert np.array_equal(y, out), (what, route)
    if route in SEQUENTIAL:
        assert log == cpu_log, (what, route)
    else:
        assert sorted(log) == sorted(keys.values()), (what, route)              # every distinct section once
    assert np.array_equal(untransform(lib, fmt, y, got), x), (what, route)
    return choice


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", SIZES)
@pytest.mark.parametrize("fmt,use_all", KINDS)
def test_every_candidate_wins_on_every_route(lib, fmt, use_all, blocks):
    _x, secs, keys = case(fmt, blocks, use_all)
    for k, (cand, _s) in enumerate(secs):
        for route in ROUTES:
            check_exact(lib, fmt, blocks, use_all, winner_table(secs, keys, k), None, route, ("winner", k), want_choice=cand)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,use_all", KINDS_123)
def test_every_candidate_wins_through_the_core_call_and_the_stable_builder(lib, fmt, use_all):
    n = FMT_ID[fmt]
    x, secs, keys = case(fmt, 129, use_all)
    for k, (cand, _s) in enumerate(secs):
        table = winner_table(secs, keys, k)
        choice, out, cpu_log, _code = cpu_auto(fmt, x, use_all, table, None)
        assert choice == cand
        # core: dltbcNcore_transform_auto reports settings, which untransform
        log = []
        est = cabi.scripted_estimator(table, None, log)
        y, st = np.full(x.size, 0xEE, dtype=np.uint8), core_settings(n, tuple(1 - c if i else c ^ 2 for i, c in enumerate(cand)))
        r = getattr(lib, f"dltbc{n}core_transform_auto")(x.ctypes.data, x.size, y.ctypes.data, y.size, C.byref(est),
                                                         cabi.AutoSettings(use_all), C.byref(st))
        assert r.ErrorCode == 0 and log == cpu_log, k
        got = (st.DecorrelationMode, int(st.SplitAlphaEndpoints) if n == 3 else 0, int(st.SplitColourEndpoints))
        assert got == cand and np.array_equal(y, out), (k, got, cand)
        z = np.zeros_like(x)
        assert getattr(lib, f"dltbc{n}core_untransform")(y.ctypes.data, y.size, z.ctypes.data, z.size, st).ErrorCode == 0
        assert np.array_equal(z, x), k
        # stable: the AutoTransformBuilder returns a manual builder, which untransforms
        p = f"dltbc{n}_"
        log = []
        est = cabi.scripted_estimator(table, None, log)
        ab = getattr(lib, p + "new_AutoTransformBuilder")(C.byref(est))
        try:
            assert getattr(lib, p + "AutoTransformBuilder_SetUseAllDecorrelationModes")(ab, use_all).ErrorCode == 0
            y, mb = np.full(x.size, 0xEE, dtype=np.uint8), C.c_void_p()
            r = getattr(lib, p + "AutoTransformBuilder_Transform")(ab, x.ctypes.data, x.size, y.ctypes.data, y.size, C.byref(mb))
            assert r.ErrorCode == 0 and mb.value and log == cpu_log, k
            assert np.array_equal(y, out), k
            z = np.zeros_like(x)
            r = getattr(lib, p + "ManualTransformBuilder_Untransform")(y.ctypes.data, y.size, z.ctypes.data, z.size, mb)
            assert r.ErrorCode == 0 and np.array_equal(z, x), k
            getattr(lib, p + "free_ManualTransformBuilder")(mb)
        finally:
            getattr(lib, p + "free_AutoTransformBuilder")(ab)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", SIZES)
@pytest.mark.parametrize("fmt,use_all", KINDS)
def test_ties_keep_the_first_minimum_on_every_route(lib, fmt, use_all, blocks):
    _x, secs, keys = case(fmt, blocks, use_all)
    tables = tie_tables(fmt, secs, keys)
    assert len(tables) == {"bc1": 1 + len(secs) * (len(secs) - 1) // 2, "bc2": 1 + len(secs) * (len(secs) - 1) // 2,
                           "bc3": 1 + (28 if use_all else 6), "bc4": 1, "bc5": 2}[fmt]
    for name, table, default in tables:
        for route in ROUTES:
            choice = check_exact(lib, fmt, blocks, use_all, table, default, route, name)
            if name == "all equal" or name == "crossed":
                assert choice == secs[0][0]


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", SIZES)
@pytest.mark.parametrize("fmt,use_all", KINDS)
def test_the_all_maximum_estimator_keeps_the_defaults_on_every_route(lib, fmt, use_all, blocks):
    x, _secs, keys = case(fmt, blocks, use_all)
    table, default = maximum_table(fmt, keys)
    for max_extra in (None, 64):                 # MaxCompressedSize answers 0 (no scratch buffer), and n + 64
        for route in ROUTES:
            check_exact(lib, fmt, blocks, use_all, table, default, route, ("maximum", max_extra), max_extra=max_extra,
                        want_choice=DEFAULTS[fmt])
    assert np.array_equal(cpu_auto(fmt, x, use_all, table, default)[1], cabi.cpu_transform(fmt, x, DEFAULTS[fmt]))


def failing_call(lib, fmt, blocks, use_all, table, default, fail_at, route, what):
    """one failing call on `route` against the CPU statement; returns the log of the library's estimator"""
    x, _secs, _keys = case(fmt, blocks, use_all)
    choice, _out, cpu_log, code = cpu_auto(fmt, x, use_all, table, default, fail_at)
    assert choice is None and code is not None, what
    log = []
    est = cabi.scripted_estimator(table, default, log, fail_at)
    with on_route(lib, route):
        rc, _got, _y, err = call_auto(lib, fmt, x, est, use_all)
    assert rc == E_ESTIMATOR, (what, route, rc)
    # the BC4 / BC5 calls have no parameter for the code: the thread's last one is read through the debug hook, for every format
    assert err in (code, None) and lib.dxtlt_debug_auto_last_estimator_error() == code, (what, route, err, code)
    if route in SEQUENTIAL:
        assert log == cpu_log, (what, route, len(log), len(cpu_log))      # the same sections up to the failure, nothing after it
    return log


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", SIZES)
@pytest.mark.parametrize("fmt,use_all", KINDS)
def test_a_failing_estimate_at_every_call_of_the_sequential_routes(lib, fmt, use_all, blocks):
    """Call k of the sequential sequence answers 100 + k: that code comes back, nothing is called after it, and the next call of the
    thread is exact -- on the staged route a download of the next candidate is in flight when the estimate fails."""
    _x, secs, keys = case(fmt, blocks, use_all)
    calls = sum(len(s) for _c, s in secs)
    for k in range(calls):
        for route in SEQUENTIAL:
            log = failing_call(lib, fmt, blocks, use_all, {}, 7, (k, 100 + k), route, ("fails at", k))
            assert len(log) == k + 1, (k, route)
            check_exact(lib, fmt, blocks, use_all, winner_table(secs, keys, k % len(secs)), None, route, ("after failure", k))


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", SIZES)
@pytest.mark.parametrize("fmt,use_all", KINDS)
def test_the_parallel_route_reports_the_failure_the_sequential_order_meets_first(lib, fmt, use_all, blocks):
    """Every section of a subset F fails with a code of its own; the call reports the one the sequential order shows first."""
    _x, secs, keys = case(fmt, blocks, use_all)
    ids = sorted(keys)
    rng = np.random.default_rng(0xFA11 + FMT_ID[fmt] * 2 + use_all)
    subsets = [[i] for i in ids] + [ids] + [list(rng.permutation(len(ids))[:2 + r % 3]) for r in range(8)]
    subsets = [[s if isinstance(s, tuple) else ids[int(s)] for s in sub] for sub in subsets]
    seen_codes = set()
    for n, sub in enumerate(subsets):
        table = {keys[i]: ("fail", 200 + ids.index(i)) if i in sub else 10 for i in ids}
        x = case(fmt, blocks, use_all)[0]
        want = cpu_auto(fmt, x, use_all, table, None)[3]
        assert want in {200 + ids.index(i) for i in sub}
        seen_codes.add(want)
        failing_call(lib, fmt, blocks, use_all, table, None, None, "threads4", ("subset", n))
        check_exact(lib, fmt, blocks, use_all, winner_table(secs, keys, n % len(secs)), None, "threads4", ("after failure", n))
    assert len(seen_codes) == len(ids)            # each section was the first failure of some subset


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", SIZES)
@pytest.mark.parametrize("use_all", [False, True])
def test_normalization_route_every_candidate_wins_and_failures_skip(lib, use_all, blocks):
    x, secs = norm_case(blocks, use_all)
    f = lib.dxtlt_transform_bc1_auto_with_normalization

    def run(table, default, what):
        log, cpu_log = [], []
        est = cabi.scripted_estimator(table, default, log)
        want, out, _calls = oracle_auto.transform_bc1_auto_with_normalization(x, cabi.scripted_estimate(table, default, cpu_log), use_all)
        want = tuple(int(c) for c in want)
        y = np.full(x.size, 0xEE, dtype=np.uint8)
        m, v, s, err = C.c_uint8(want[0] ^ 0x80), C.c_uint8(want[1] ^ 0x80), C.c_bool(not want[2]), C.c_uint32(0xEEEE)
        rc = f(x.ctypes.data, y.ctypes.data, x.size, C.byref(est), use_all, C.byref(m), C.byref(v), C.byref(s), C.byref(err))
        assert rc == 0 and err.value == 0, (what, rc, err.value)
        got = (m.value, v.value, int(s.value))
        assert got == want and np.array_equal(y, out) and log == cpu_log, (what, got, want)
        assert log == [key for _c, key in secs], what                          # every candidate is tried, failing ones too
        z = untransform(lib, "bc1", y, (got[1], 0, got[2]))
        assert np.array_equal(z, oracle_c.normalize_bc1_blocks(x, got[0]) if got[0] else x), what
        return got

    for k, (cand, key) in enumerate(secs):
        table = {other: 20 for _c, other in secs}
        table[key] = 10
        assert run(table, None, ("winner", k)) == cand
        # every estimate fails but this one, which answers one below the maximum: it wins
        assert run({key: SIZE_MAX - 1}, ("fail", 9), ("lone survivor", k)) == cand
    assert run({}, ("fail", 9), "all fail") == (0, 1, 1)
    assert run({}, SIZE_MAX, "all maximum") == (0, 1, 1)
    assert run({}, 7, "all equal") == secs[0][0]
