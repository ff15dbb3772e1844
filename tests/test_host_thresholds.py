"""Every arm of the host-pointer round trip and of the sharded worker on buffers of a few MiB.

The host paths choose between the mapped pinned pair, the one-shot H2D + kernel + D2H and the chunked pipeline by
thresholds that are read once per process (DXTLT_MAPPED_MAX_BYTES, DXTLT_PIPELINE_MIN_BYTES, DXTLT_PIPELINE_CHUNK_BYTES).
With the shipped values a test buffer below 96 MiB never reaches the pipeline, so each environment below gets a child
process of its own (this file, run as a script), which checks the host-pointer call and the sharded call (three shards;
for BC6H / BC7 the last one holds the granule tail) of formats 1, 3, 5, 6 and 7 against the CPU statements, forward and
inverse, at a size of several 1 MiB chunks plus an odd rest and at a size below 1 MiB."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENVIRONMENTS = {
    # pipeline from 1 MiB up in 1 MiB chunks: whole buffers and every shard go through upload | kernel | download
    "pipeline": {"DXTLT_PIPELINE_MIN_BYTES": "1048576", "DXTLT_PIPELINE_CHUNK_BYTES": "1048576"},
    # mapped staging off (1 byte): small and large buffers alike take the one-shot copies, shards the per-slice copies
    "one_shot": {"DXTLT_MAPPED_MAX_BYTES": "1"},
}
FORMATS = ("bc1", "bc3", "bc5", "bc6h", "bc7")
BLOCK = {"bc1": 8, "bc3": 16, "bc5": 16, "bc6h": 16, "bc7": 16}
# ~10.7 MiB: ten chunks and a rest per buffer, three and a rest per shard; 700 001 = 683 granules + 609 blocks of tail
LARGE_BYTES = 700_001 * 16
SMALL_BLOCKS = 4099


def cases(pkg, oracle):
    """(format, forward(x, y), inverse(y, z), sharded(inverse, src, dst), blocks -> (input, expected transform))"""
    import bc45_ref
    import bc6h_ref
    from dxt_lossless_transform_amd import bc6h, bc7
    from tests.test_bc6h_gpu import blocks_of
    from tests.test_bc7 import make_blocks

    def random_blocks(fmt, n):
        return np.random.default_rng(n + BLOCK[fmt]).integers(0, 256, n * BLOCK[fmt], dtype=np.uint8)

    def block_format(fmt, st, want):
        def make(n):
            x = random_blocks(fmt, n)
            return x, want(x)

        return (fmt, lambda x, y: getattr(pkg, f"transform_{fmt}_with_settings")(x, y, st),
                lambda y, z: getattr(pkg, f"untransform_{fmt}_with_settings")(y, z, st),
                lambda inverse, s, d: pkg.transform_sharded(fmt, inverse, s, d, st, 3), make)

    def granule_format(fmt, mod, make):
        return (fmt, getattr(mod, f"transform_{fmt}"), getattr(mod, f"untransform_{fmt}"),
                lambda inverse, s, d: getattr(mod, f"transform_{fmt}_sharded")(s, d, 3, inverse=inverse), make)

    def bc6h_blocks(n):
        x = blocks_of(n, "uniform", n)
        return x, bc6h_ref.transform(x)

    def bc7_blocks(n):
        x = make_blocks(oracle, n, "uniform", n)
        return x, oracle.transform_bc7(x)

    st1 = pkg.Bc1TransformSettings(pkg.YCoCgVariant(2), True)
    st3 = pkg.Bc3TransformSettings(pkg.YCoCgVariant(1), True, True)
    return [
        block_format("bc1", st1, lambda x: oracle.transform("bc1", x, 2, True, True)),
        block_format("bc3", st3, lambda x: oracle.transform("bc3", x, 1, True, True)),
        block_format("bc5", pkg.Bc5TransformSettings(True), lambda x: bc45_ref.transform("bc5", x, True)),
        granule_format("bc6h", bc6h, bc6h_blocks),
        granule_format("bc7", bc7, bc7_blocks),
    ]


def check_all():
    """The child process: the thresholds are whatever its environment says."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import dxt_lossless_transform_amd as pkg
    from oracle import oracle_c

    pkg.load()
    oracle_c.lib()
    seen = []
    for fmt, forward, inverse, sharded, make in cases(pkg, oracle_c):
        for n in (LARGE_BYTES // BLOCK[fmt], SMALL_BLOCKS):
            x, want = make(n)
            for name, fwd, inv in (("host", forward, inverse),
                                   ("sharded", lambda s, d: sharded(False, s, d), lambda s, d: sharded(True, s, d))):
                y, z = np.full_like(x, 0xEE), np.full_like(x, 0xEE)
                fwd(x, y)
                assert np.array_equal(y, want), (fmt, n, name, "forward differs from the CPU statement")
                inv(want, z)
                assert np.array_equal(z, x), (fmt, n, name, "inverse differs from the CPU statement")
                seen.append((fmt, n, name))
    assert len(seen) == len(FORMATS) * 2 * 2
    print(f"checked {len(seen)} (format, size, path) cases, forward and inverse")


@pytest.mark.gpu
def test_host_and_sharded_paths_under_thresholds(pkg):
    for name, settings in sorted(ENVIRONMENTS.items()):
        env = {k: v for k, v in os.environ.items() if not k.startswith(("DXTLT_PIPELINE_", "DXTLT_MAPPED_"))}
        env.update(settings)
        done = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True,
                              timeout=900)
        assert done.returncode == 0, f"{name}: exit {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}"
        assert "checked 20 " in done.stdout, (name, done.stdout[-2000:])


if __name__ == "__main__":
    check_all()
