"""Every stream layout the library can build, through every arm of the host-pointer round trip and of the sharded worker.

tests/test_host_thresholds.py forces the pipeline and the one-shot copies on five layouts at one setting each; here every
distinct StreamLayout -- BC1 / BC2 with and without the colour split, all four BC3 splits, BC4 / BC5 with and without the
endpoint split, BC6H, BC7, 3- and 4-byte pixels interleaved, planar and planar-delta, and the BC1 transform with fused block
normalisation -- passes through the mapped pair, the one-shot copies and a 64 KiB-chunk pipeline, as a whole buffer and in
shards, at the smallest sizes that cross every chunk, shard and tail boundary (tests/host_paths_cases.py).  The thresholds are
read once per process, so each environment is a child process (this file, run as a script).  Every case compares both
directions with the CPU statement byte for byte, inside guard bytes, and compares dxtlt_debug_host_route_counts around each
call with the route the documented rules predict: a case that silently takes another arm fails.

A 3-byte-pixel buffer of one chunk and one pixel (20 481 pixels = 61 443 bytes) stays below the 64 KiB pipeline threshold and
is predicted -- and checked -- as a one-shot copy; its other sizes are pipelined in chunks of 20 480 pixels."""
import os
import subprocess
import sys

import pytest

import host_paths_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_all(env_name):
    """The child process: the thresholds are whatever its environment says."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import dxt_lossless_transform_amd as pkg
    from oracle import oracle_c

    pkg.load()
    oracle_c.lib()
    return H.run_all(env_name, pkg, oracle_c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(H.ENVIRONMENTS))
def test_every_layout_on_every_staging_arm(pkg, name):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("DXTLT_PIPELINE_", "DXTLT_MAPPED_"))}
    env.update(H.ENVIRONMENTS[name])
    done = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, cwd=ROOT, capture_output=True, text=True,
                          timeout=900)
    print(done.stdout[-3000:])
    assert done.returncode == 0, f"{name}: exit {done.returncode}\n{done.stdout[-6000:]}\n{done.stderr[-4000:]}"
    assert f"checked {H.case_count()} (layout, size, path) cases" in done.stdout, (name, done.stdout[-2000:])


# ---- no device ------------------------------------------------------------------------------------------------------------------
def reachable_layouts(pkg):
    """{(format, unit bytes, stream table)} of every StreamLayout a caller can reach: formats 1-5 from every combination of their
    settings, the granule formats' one table (docs/BC7_FORMAT.md, docs/BC6H_FORMAT.md; tests/bc6h_ref.py), and the pixel
    layouts of docs/PIXEL_FORMAT.md for both pixel sizes."""
    import bc6h_ref
    import pixels_ref

    out = set()
    for fmt, unit in pkg.BLOCK_BYTES.items():
        for st in getattr(pkg, f"Bc{fmt[2]}TransformSettings").all_combinations():
            out.add((fmt, unit, tuple(pkg.stream_table(fmt, st))))
    granule = tuple(zip(bc6h_ref.STREAM_OFF, bc6h_ref.STREAM_WIDTH))
    out |= {("bc6h", 16, granule), ("bc7", 16, granule)}
    for B in (3, 4):
        for layout in pixels_ref.LAYOUTS:
            out.add((f"pixels{B}", B, ((0, B),) if layout == pixels_ref.INTERLEAVED else tuple((c, 1) for c in range(B))))
    return out, granule


def test_case_table_covers_every_reachable_layout_on_every_arm(pkg):
    import pixels_ref

    reachable, granule = reachable_layouts(pkg)
    assert len(reachable) == 2 + 2 + 4 + 2 + 2 + 2 + 4
    for env in H.ENVIRONMENTS:
        assert set(H.ENVIRONMENTS[env]) <= {"DXTLT_MAPPED_MAX_BYTES", "DXTLT_PIPELINE_MIN_BYTES", "DXTLT_PIPELINE_CHUNK_BYTES"}
        # the arm a whole buffer and a shard must reach under this environment, for every layout
        host_arm = {"pipeline": H.PIPELINED, "one_shot": H.ONE_SHOT, "default": H.MAPPED}[env]
        shard_arm = H.PIPELINED if env == "pipeline" else H.SHARD_ONE_SHOT
        covered = {}
        for case in H.ordered_cases():
            L = case.layout
            key = (L.fmt if L.family != "normalize" else "bc1", L.unit, H.stream_table(L, pkg, granule))
            counts = H.expected_counts(env, case)
            arm = host_arm if case.path == "host" else shard_arm
            if counts[arm]:
                covered.setdefault(key, set()).add(case.path)
            assert case.units * L.unit < H.MIB, "the sizes stay below the mapped pair's 1 MiB"
            # exactly one arm per round trip; chunks only with the pipeline; host calls never count shard transfers
            assert (counts[H.CHUNKS] > 0) == (counts[H.PIPELINED] > 0)
            if case.path == "host":
                assert counts[H.SHARD_ONE_SHOT] == 0 and 1 <= counts[H.MAPPED] + counts[H.ONE_SHOT] + counts[H.PIPELINED] <= 2
            else:
                nonempty = sum(1 for _, n in H.plan_shards(L, case.units, case.shards) if n)
                tail_shot = counts[H.PIPELINED] and L.family == "granule" and case.units % H.GRANULE != 0
                assert counts[H.MAPPED] == counts[H.ONE_SHOT] == 0
                assert counts[H.PIPELINED] + counts[H.SHARD_ONE_SHOT] == nonempty + (1 if tail_shot else 0)
        missing = {k: {"host", "sharded"} - covered.get(k, set()) for k in reachable if covered.get(k, set()) != {"host", "sharded"}}
        assert not missing, (env, "layouts without a case on the environment's arm", missing)
        assert set(covered) == reachable, (env, "cases of a layout the library cannot build", set(covered) - reachable)
    # the settings the layouts do not show: a non-zero decorrelation variant per colour format, both pixel decorrelation
    # settings, every pixel layout for both sizes, both normalisation modes
    ls = H.layouts()
    for fmt in ("bc1", "bc2", "bc3"):
        assert any(L.fmt == fmt and L.family == "block" and L.settings[0] != 0 for L in ls)
    for B in (3, 4):
        seen = {L.settings for L in ls if L.family == "pixel" and L.unit == B}
        assert {s[1] for s in seen} == set(pixels_ref.LAYOUTS) and {s[0] for s in seen} == {False, True}
        assert (True, pixels_ref.PLANAR_DELTA) in seen and (False, pixels_ref.PLANAR_DELTA) in seen
    assert {L.settings[0] for L in ls if L.family == "normalize"} == {1, 2}
    assert all(L.settings[2] for L in ls if L.family == "normalize")
    assert len(H.ordered_cases()) == H.case_count() == 20 * 7 + 2 * 9 + 2 * 4


def test_chunk_counts_follow_the_documented_rule():
    """64 KiB chunks: floor(65536 / unit) rounded down to the alignment -- 20 480 pixels of 3 bytes, not 21 845"""
    chunk = {L.name: H.chunk_units(L) for L in H.layouts()}
    for L in H.layouts():
        want = {("block", 8): 8192, ("normalize", 8): 8192, ("block", 16): 4096, ("granule", 16): 4096, ("pixel", 4): 16384,
                ("pixel", 3): 20480}[(L.family, L.unit)]
        assert chunk[L.name] == want and want % L.align == 0
        C, A = want, L.align
        assert L.align == {"block": 2048, "normalize": 2048, "granule": 1024, "pixel": 4096}[L.family]
        if L.family == "granule":
            assert H.host_sizes(L) == [3 * C, 3 * C + 1, 3 * C + 1023, C + 1024, C + 1025, C + 2047]
            chunks = [3, 3, 3, 2, 2, 2]
            trips = [1, 2, 2, 1, 2, 2]      # with a tail part: the whole granules pipelined, then the tail as one shot
        else:
            assert H.host_sizes(L) == [3 * C, 3 * C + 1, C + 1, 2 * C + A - 1]
            # one chunk and one pixel of 3 bytes is 61 443 bytes: below the 64 KiB threshold, one shot
            chunks = [3, 4, 0 if L.unit == 3 else 2, 3]
            trips = [1, 1, 1, 1]
        for n, want_chunks, want_trips in zip(H.host_sizes(L), chunks, trips):
            counts = H.expected_counts("pipeline", H.Case(L, "host", n, 0))
            assert counts[H.CHUNKS] == want_chunks, (L.name, n, counts)
            assert counts[H.PIPELINED] == (1 if want_chunks else 0) and counts[H.ONE_SHOT] == want_trips - counts[H.PIPELINED]
            assert H.expected_counts("one_shot", H.Case(L, "host", n, 0)) == [0, 1, 0, 0, 0]
            assert H.expected_counts("default", H.Case(L, "host", n, 0)) == [1, 0, 0, 0, 0]
        if L.family == "normalize":
            continue
        big, everything_in_last, many = [H.Case(L, "sharded", n, shards) for shards, n in H.sharded_sizes(L)]
        assert H.plan_shards(L, big.units, 3) == [(0, 2 * C + A), (2 * C + A, 2 * C + A), (4 * C + 2 * A, 2 * C + A + 5)]
        # three pipelined shards of two chunks and a rest; the granule formats' 5 ragged blocks are the last shard's tail part
        assert H.expected_counts("pipeline", big) == [0, 0, 3, 9, 1 if L.family == "granule" else 0]
        assert H.expected_counts("one_shot", big) == H.expected_counts("default", big) == [0, 0, 0, 0, 3]
        assert H.plan_shards(L, everything_in_last.units, 3) == [(0, 0), (0, 0), (0, 2 * A + 3)]
        plan = H.plan_shards(L, many.units, 64)
        assert len(plan) == (64 if L.shard_unit == 1 else 6) and plan[-1] == (0, 5 * A + 1)
        for case in (everything_in_last, many):
            whole = case.units - (case.units % H.GRANULE if L.family == "granule" else 0)
            if whole * L.unit >= H.CHUNK_BYTES:
                want = [0, 0, 1, -(-whole // C), 1 if whole != case.units else 0]
            else:
                want = [0, 0, 0, 0, 1]
            assert H.expected_counts("pipeline", case) == want, (L.name, case.units)
            assert H.expected_counts("default", case) == [0, 0, 0, 0, 1]


if __name__ == "__main__":
    sys.exit(check_all(sys.argv[1]))
