"""BC2 / BC3 block normalisation fused into the forward transform, on the device, under byte comparison
(dxtlt_transform_bc{2,3}_with_normalize_blocks[_device], include/dxtlt_bc23_normalize.h; kernels: csrc/bcn_norm23_kernels.hip).

Case lists, data and expectations are those of tests/test_normalize_fused_bc23.py, which shows without a device what they reach:
expected bytes are always oracle.transform(fmt, oracle.normalize_bcN_blocks(x, modes), settings).  Every device arena carries 256
guard bytes (test_alignment_sweep.GUARD) around every output; they are checked after the run, and so is that the input is unchanged.

1. Residue sweep: the BC2 / BC3 forward whole-buffer cases of test_alignment_sweep.build_cases (all 128 SoA residues x its counts
   for the default and the all-off settings, its subset for the others), colour mode 2 on BC2, mode pair (3, 2) on BC3.
2. Every mode pair (2 for BC2, 11 for BC3) on the default and the all-off settings at 1, T - 1, T, T + 1, 2T + 9, 3T blocks
   (T = 256, the aligned tile), SoA residues 0 and 1.
3. Forced forms: set_tuning(0, 0x2 | 0x20 | 0x22) at 3T on residues 0 and 64, for every kernel set, restored afterwards.
4. Mode pair (None, None) equals the plain device transform byte for byte.
5. Round trip: untransform of the fused output is the oracle's normalize_blocks of the input, one case per kernel set.
6. Host calls: 4 KiB + 16 bytes takes the mapped route, 1 MiB + 16 bytes the upload route, and one BC3 case runs the chunked
   pipeline at a small size in a child process under host_paths_cases.ENVIRONMENTS["pipeline"] (the thresholds are read once
   per process).
7. HIP graph: one BC3 device call captured on a stream and replayed twice gives the bytes of the eager call.
8. The Python wrappers and the C++ mirror (tests/cpp/test_cpp_normalize_fused_bc23.cpp, built the way tests/test_cpp_api.py builds
   its file) against the C ABI's bytes.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                       # (the child process of the pipeline case runs this file as a script)
    sys.path.insert(0, ROOT)

import host_paths_cases as H  # noqa: E402
from helpers import pkg_settings  # noqa: E402
from test_alignment_sweep import ALL_OFF, DEFAULT, SETTINGS, Arena, dev, device_arena, group_of, lib, verify  # noqa: E402, F401
from test_normalize_fused_bc23 import (FORCED, FORMATS, HOST_COUNTS, MODE_PAIRS, PAIR_COUNTS, SWEEP_MODES, T, blocks_of, bound, expected,
                                       forced_cases, normalized, pair_cases, round_trip_case, sweep_cases)  # noqa: E402


@pytest.fixture(scope="module")
def norm(pkg):
    from dxt_lossless_transform_amd import normalize as mod

    return mod


def fused(norm, fmt, src, dst, modes, s):
    if fmt == "bc2":
        norm.transform_bc2_with_normalize_blocks(src, dst, modes[1], s[0], bool(s[2]))
    else:
        norm.transform_bc3_with_normalize_blocks(src, dst, modes[0], modes[1], s[0], bool(s[1]), bool(s[2]))


def run_fused(pkg, norm, oracle, lib, dev, fmt, modes, s, launches, label):
    """launches: [(case, force bits)], each into its own slot of one 0xA5 arena at the case's SoA residue, reading its input at the
    case's AoS residue; one download: outputs == CPU statement, guards intact, inputs unchanged"""
    import torch

    a_in, a_out = Arena(), Arena()
    in_at = {}
    for c, _ in launches:
        if (c.num, c.a) not in in_at:
            in_at[(c.num, c.a)] = a_in.place(c.a, c.num * 16)
    h_in = np.zeros(a_in.size(), dtype=np.uint8)
    for (n, a), off in in_at.items():
        h_in[off:off + n * 16] = blocks_of(oracle, fmt, n)
    d_in = device_arena(dev, h_in.size, 0)
    d_in.copy_(torch.from_numpy(h_in))
    out_at = [a_out.place(c.p, c.num * 16) for c, _ in launches]
    d_out = device_arena(dev, a_out.size(), 0xA5)
    force_now = 0
    try:
        for (c, f), o in zip(launches, out_at):
            if f != force_now:
                pkg.set_tuning(0, f)
                force_now = f
            i = in_at[(c.num, c.a)]
            fused(norm, fmt, d_in[i:i + c.num * 16], d_out[o:o + c.num * 16], modes, s)
    finally:
        pkg.set_tuning(0, 0)
    torch.cuda.synchronize()
    got_out, got_in = d_out.cpu().numpy(), d_in.cpu().numpy()
    verify(lib, got_out, d_out.data_ptr(), 0xA5, [(o, expected(oracle, fmt, s, c.num, modes), c) for (c, _), o in zip(launches, out_at)],
           label, lambda c: d_in.data_ptr() + in_at[(c.num, c.a)])
    assert np.array_equal(got_in, h_in), (label, "the fused transform changed its input")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_transform_at_every_residue(pkg, norm, oracle, lib, dev, fmt):
    assert [c for s in SETTINGS[fmt] for c in group_of(fmt, s, False, True)] == sweep_cases(fmt)
    for s in SETTINGS[fmt]:
        run_fused(pkg, norm, oracle, lib, dev, fmt, SWEEP_MODES[fmt], s, [(c, 0) for c in group_of(fmt, s, False, True)],
                  f"{fmt} fused modes {SWEEP_MODES[fmt]} v{s[0]}-sa{s[1]}-sc{s[2]}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_transform_with_every_mode_pair(pkg, norm, oracle, lib, dev, fmt):
    cases = pair_cases(fmt)
    assert {c.num for c in cases} == set(PAIR_COUNTS) and {c.p for c in cases} == {0, 1}
    for modes in MODE_PAIRS[fmt]:
        for s in (DEFAULT[fmt], ALL_OFF):
            run_fused(pkg, norm, oracle, lib, dev, fmt, modes, s, [(c, 0) for c in cases if c.settings == s],
                      f"{fmt} fused modes {modes} v{s[0]}-sa{s[1]}-sc{s[2]}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_transform_forced_forms(pkg, norm, oracle, lib, dev, fmt):
    """halo tiles for aligned bases (2), the generic LDS form for natural shifts (0x20), both (0x22), for every kernel set"""
    for s in SETTINGS[fmt]:
        run_fused(pkg, norm, oracle, lib, dev, fmt, SWEEP_MODES[fmt], s, [(c, f) for f in FORCED for c in forced_cases(fmt, s)],
                  f"{fmt} fused v{s[0]}-sa{s[1]}-sc{s[2]}, forced forms 0x2, 0x20, 0x22 in thirds (the plan shown is the unforced one)")
    assert pkg.tuning_mask() & 0x22 == 0x22


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_mode_pair_none_is_the_plain_transform(pkg, norm, oracle, lib, dev, fmt):
    """(None, None) through the fused entry points == dxtlt_transform_bcN_with_settings_device, byte for byte, and == the oracle's
    plain transform of the un-normalised input"""
    import torch

    plain = getattr(pkg, f"transform_{fmt}_with_settings")
    for s in (DEFAULT[fmt], ALL_OFF):
        cases = [c for c in pair_cases(fmt) if c.settings == s]
        run_fused(pkg, norm, oracle, lib, dev, fmt, (0, 0), s, [(c, 0) for c in cases], f"{fmt} fused modes (None, None)")
        for n in PAIR_COUNTS:
            x = torch.from_numpy(blocks_of(oracle, fmt, n).copy()).to(dev)
            a, b = torch.zeros_like(x), torch.zeros_like(x)
            fused(norm, fmt, x, a, (0, 0), s)
            plain(x, b, pkg_settings(pkg, fmt, s))
            torch.cuda.synchronize()
            assert torch.equal(a, b), (fmt, s, n)
            assert np.array_equal(a.cpu().numpy(), oracle.transform(fmt, blocks_of(oracle, fmt, n), s[0], bool(s[2]), bool(s[1])))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_untransform_yields_the_normalised_blocks(pkg, norm, oracle, dev, fmt):
    import torch

    inverse = getattr(pkg, f"untransform_{fmt}_with_settings")
    modes = SWEEP_MODES[fmt]
    for s in SETTINGS[fmt]:
        c = round_trip_case(fmt, s)
        a_soa, a_aos = Arena(), Arena()
        o_soa, o_aos = a_soa.place(c.p, c.num * 16), a_aos.place(c.a, c.num * 16)
        x = torch.from_numpy(blocks_of(oracle, fmt, c.num).copy()).to(dev)
        d_soa, d_aos = device_arena(dev, a_soa.size(), 0xA5), device_arena(dev, a_aos.size(), 0x5A)
        fused(norm, fmt, x, d_soa[o_soa:o_soa + c.num * 16], modes, s)
        inverse(d_soa[o_soa:o_soa + c.num * 16], d_aos[o_aos:o_aos + c.num * 16], pkg_settings(pkg, fmt, s))
        torch.cuda.synchronize()
        want = np.full(a_aos.size(), 0x5A, dtype=np.uint8)
        want[o_aos:o_aos + c.num * 16] = normalized(oracle, fmt, c.num, modes)
        assert np.array_equal(d_aos.cpu().numpy(), want), (fmt, s, "untransform(fused) != normalize_blocks(input)")
        assert not np.array_equal(normalized(oracle, fmt, c.num, modes), blocks_of(oracle, fmt, c.num))


def guarded(n):
    """n bytes with 256 guard bytes of 0xA5 on both sides, in host memory"""
    whole = np.full(n + 512, 0xA5, dtype=np.uint8)
    return whole, whole[256:256 + n]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_calls_take_the_mapped_and_the_upload_route(pkg, norm, oracle, fmt):
    assert HOST_COUNTS[0] * 16 == 4096 + 16 and HOST_COUNTS[1] * 16 == (1 << 20) + 16
    for n, route in zip(HOST_COUNTS, (H.MAPPED, H.ONE_SHOT)):
        for modes, s in ((SWEEP_MODES[fmt], DEFAULT[fmt]), (MODE_PAIRS[fmt][0], ALL_OFF)):
            x = blocks_of(oracle, fmt, n)
            keep = x.copy()
            whole, out = guarded(x.size)
            before = pkg.host_route_counts()
            fused(norm, fmt, x, out, modes, s)
            after = pkg.host_route_counts()
            delta = [int(b) - int(a) for a, b in zip(before, after)]
            assert delta == [1 if k == route else 0 for k in range(len(delta))], (fmt, n, delta)
            assert np.array_equal(out, expected(oracle, fmt, s, n, modes)), (fmt, n, modes, s)
            assert (whole[:256] == 0xA5).all() and (whole[-256:] == 0xA5).all() and np.array_equal(x, keep)


PIPELINE_BLOCKS = 2 * (H.CHUNK_BYTES // 16) + 777             # two whole 64 KiB chunks and a ragged third


def pipeline_child():
    """(run as a script, under ENVIRONMENTS["pipeline"]) one BC3 fused host call through the chunked pipeline; prints a JSON line"""
    import dxt_lossless_transform_amd as pkg
    from dxt_lossless_transform_amd import normalize as norm
    from oracle import oracle_c as oracle

    modes, s = SWEEP_MODES["bc3"], DEFAULT["bc3"]
    x = blocks_of(oracle, "bc3", HOST_COUNTS[1])[:PIPELINE_BLOCKS * 16]
    want = oracle.transform("bc3", oracle.normalize_bc3_blocks(x, *modes), s[0], bool(s[2]), bool(s[1]))
    whole, out = guarded(x.size)
    before = pkg.host_route_counts()
    fused(norm, "bc3", x, out, modes, s)
    after = pkg.host_route_counts()
    print(json.dumps({"delta": [int(b) - int(a) for a, b in zip(before, after)], "equal": bool(np.array_equal(out, want)),
                      "guards": bool((whole[:256] == 0xA5).all() and (whole[-256:] == 0xA5).all()),
                      "differs_from_plain": not np.array_equal(want, oracle.transform("bc3", x, s[0], bool(s[2]), bool(s[1])))}))


@pytest.mark.gpu
def test_host_call_through_the_chunked_pipeline(pkg):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("DXTLT_PIPELINE_", "DXTLT_MAPPED_"))}
    env.update(H.ENVIRONMENTS["pipeline"])
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "pipeline"], env=env, cwd=ROOT, capture_output=True, text=True,
                          timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    r = json.loads(done.stdout.strip().splitlines()[-1])
    assert r["equal"] and r["guards"] and r["differs_from_plain"], r
    assert r["delta"][H.MAPPED] == 0 and r["delta"][H.ONE_SHOT] == 0 and r["delta"][H.PIPELINED] == 1 and r["delta"][H.CHUNKS] == 3, r


@pytest.mark.gpu
def test_device_call_replays_from_a_hip_graph(pkg, norm, oracle, dev):
    """One BC3 device call (halo tiles: one kernel node) captured on a stream, replayed twice on new inputs in the same buffers"""
    import torch

    modes, s, n = SWEEP_MODES["bc3"], DEFAULT["bc3"], 2 * T + 9
    first, second = blocks_of(oracle, "bc3", n), blocks_of(oracle, "bc3", 3 * T)[:n * 16]
    assert not np.array_equal(first, second)
    x = torch.from_numpy(first.copy()).to(dev)
    y = torch.zeros_like(x)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fused(norm, "bc3", x, y, modes, s)         # warm-up outside capture (module load, first launch)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    eager = y.cpu().numpy()
    assert np.array_equal(eager, expected(oracle, "bc3", s, n, modes))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused(norm, "bc3", x, y, modes, s)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert np.array_equal(y.cpu().numpy(), eager)
    x.copy_(torch.from_numpy(second.copy()))
    y.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    want = oracle.transform("bc3", oracle.normalize_bc3_blocks(second, *modes), s[0], bool(s[2]), bool(s[1]))
    assert np.array_equal(y.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_python_wrappers_and_c_abi_agree(pkg, norm, oracle, dev, fmt):
    """the C ABI called directly (host and device entry points) and the Python wrapper, on one buffer"""
    import torch

    l = bound(pkg)
    modes, s, n = SWEEP_MODES[fmt], DEFAULT[fmt], T + 1
    x = blocks_of(oracle, fmt, n).copy()
    host, devout = np.zeros_like(x), torch.zeros(x.size, dtype=torch.uint8, device=dev)
    d_x = torch.from_numpy(x).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if fmt == "bc2":
        assert l.dxtlt_transform_bc2_with_normalize_blocks(x.ctypes.data, host.ctypes.data, x.size, modes[1], s[0], bool(s[2])) == 0
        assert l.dxtlt_transform_bc2_with_normalize_blocks_device(d_x.data_ptr(), devout.data_ptr(), x.size, modes[1], s[0], bool(s[2]),
                                                                  stream) == 0
    else:
        assert l.dxtlt_transform_bc3_with_normalize_blocks(x.ctypes.data, host.ctypes.data, x.size, modes[0], modes[1], s[0], bool(s[1]),
                                                           bool(s[2])) == 0
        assert l.dxtlt_transform_bc3_with_normalize_blocks_device(d_x.data_ptr(), devout.data_ptr(), x.size, modes[0], modes[1], s[0],
                                                                  bool(s[1]), bool(s[2]), stream) == 0
    torch.cuda.synchronize()
    py = np.zeros_like(x)
    fused(norm, fmt, x, py, modes, s)
    assert np.array_equal(host, expected(oracle, fmt, s, n, modes))
    assert np.array_equal(devout.cpu().numpy(), host) and np.array_equal(py, host)


@pytest.mark.gpu
def test_cpp_mirror_agrees_with_the_c_abi(pkg, norm, oracle, tmp_path):
    libdir = os.path.dirname(pkg._lib.lib_path())
    exe = str(tmp_path / "test_cpp_normalize_fused_bc23")
    src = os.path.join(ROOT, "tests", "cpp", "test_cpp_normalize_fused_bc23.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, src, f"-L{libdir}",
                           "-ldxtlt_gfx950", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    n = T + 1
    for fmt in FORMATS:
        modes, s = SWEEP_MODES[fmt], DEFAULT[fmt]
        x = blocks_of(oracle, fmt, n)
        (tmp_path / "in.bin").write_bytes(x.tobytes())
        r = subprocess.run([exe, fmt, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(modes[0]), str(modes[1]), str(s[0]), str(s[1]),
                            str(s[2])], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
        c_abi = np.zeros_like(x)
        fused(norm, fmt, x, c_abi, modes, s)
        assert np.array_equal(got, c_abi) and np.array_equal(got, expected(oracle, fmt, s, n, modes)), fmt


if __name__ == "__main__":
    assert sys.argv[1:] == ["pipeline"]
    pipeline_child()
