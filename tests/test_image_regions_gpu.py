"""Several images of one buffer on the MI355X (include/dxtlt_image.h: dxtlt_untransform_decode_images_device,
dxtlt_decode_images_device, dxtlt_untransform_decode_images) against the CPU statement -- the oracle's decoder rearranged into
rows, the oracle's transform for the input -- with exact equality everywhere, and against the single-image fused call level by
level.  Every input and every output sits inside 0xA5 guards and every output is prefilled with 0xA5: the guards, the pitch
padding and the bytes behind each image's last row must still be 0xA5 afterwards, and the source is unchanged.  The largest
image is 260 pixels wide."""
import numpy as np
import pytest

from image_regions_common import (BPP, CHAIN_256, CHAIN_260, CUBE, FMT_ID, FMTS, GAPS, GUARD, OK, PER_LAUNCH, TOTAL_256,
                                  TOTAL_260, Guarded, blocks_of, default_settings, expected_buffer, image_of, load, other_settings,
                                  planned_kinds, reference, region_array, region_end, settings_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


def default_pitches(fmt, regions):
    return [BPP[fmt] * w for _, w, _ in regions]


def outputs(dev, regions, pitches, out_offs=None):
    out_offs = out_offs or [0] * len(regions)
    return [Guarded(dev, pitches[i] * h if w and h else 0, out_offs[i]) for i, (_, w, h) in enumerate(regions)]


def run_regions(lib, dev, fmt, data, total, regions, settings=None, pitches=None, out_offs=None, in_off=0):
    """one call -- the fused one, or with settings None the plain decoder -- over `data`; returns every region's output bytes"""
    import torch

    pitches = pitches or default_pitches(fmt, regions)
    src = Guarded(dev, data.size, in_off, data)
    dst = outputs(dev, regions, pitches, out_offs)
    arr = region_array(regions, [d.ptr for d in dst], pitches)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        if settings is None:
            rc = lib.dxtlt_decode_images_device(FMT_ID[fmt], src.ptr, total, arr, len(regions), stream)
        else:
            rc = lib.dxtlt_untransform_decode_images_device(FMT_ID[fmt], src.ptr, total, arr, len(regions), settings[0], settings[1],
                                                            settings[2], stream)
    assert rc == OK
    torch.cuda.synchronize()
    assert np.array_equal(src.bytes(), data), "the source buffer changed"
    return [d.bytes() for d in dst]


def run_single(lib, dev, fmt, transformed, total, region, settings, pitch):
    """the single-image fused call for one region"""
    import torch

    first, width, height = region
    src = Guarded(dev, transformed.size, 0, transformed)
    dst = Guarded(dev, pitch * height)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        if fmt in ("bc4", "bc5"):
            rc = lib.dxtlt_untransform_decode_channel_image_device(FMT_ID[fmt], src.ptr, total, first, width, height, settings[1],
                                                                   dst.ptr, pitch, stream)
        else:
            rc = lib.dxtlt_untransform_decode_image_device(FMT_ID[fmt], src.ptr, total, first, width, height, settings[0], settings[1],
                                                           settings[2], dst.ptr, pitch, stream)
    assert rc == OK
    torch.cuda.synchronize()
    return dst.bytes()


def wanted(oracle, fmt, total, regions, pitches=None, seed=0):
    pitches = pitches or default_pitches(fmt, regions)
    return [expected_buffer(image_of(oracle, fmt, total, r, seed), pitches[i]) if r[1] and r[2] else np.zeros(0, np.uint8)
            for i, r in enumerate(regions)]


def assert_all_equal(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, "region", i)


# ---- case 1: chains on shifted tiles -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default", "other"])
@pytest.mark.parametrize("chain", ["256", "260x136"])
@pytest.mark.parametrize("fmt", FMTS)
def test_whole_chain_in_one_call(lib, dev, oracle, fmt, chain, which):
    settings = default_settings(fmt) if which == "default" else other_settings(fmt)
    regions, total = (CHAIN_256, TOTAL_256) if chain == "256" else (CHAIN_260, TOTAL_260)
    if chain == "256":
        assert total == 5463 and planned_kinds(lib, fmt, settings, 256, total, 0, total) == [2]   # an odd total: one shifted launch
    x, t = reference(oracle, fmt, total, settings)
    want = wanted(oracle, fmt, total, regions)
    got = run_regions(lib, dev, fmt, t, total, regions, settings)
    assert_all_equal(got, want, (fmt, chain, settings))
    for k, region in enumerate(regions):
        single = run_single(lib, dev, fmt, t, total, region, settings, BPP[fmt] * region[1])
        assert np.array_equal(got[k], single), ("the single-image call differs", fmt, chain, k)


# ---- case 2: every setting ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_chain_with_every_setting(lib, dev, oracle, fmt):
    combos = settings_of(fmt)
    assert len(combos) == {"bc1": 8, "bc2": 8, "bc3": 16, "bc4": 2, "bc5": 2}[fmt]
    want = wanted(oracle, fmt, TOTAL_260, CHAIN_260)
    for settings in combos:
        x, t = reference(oracle, fmt, TOTAL_260, settings)
        assert_all_equal(run_regions(lib, dev, fmt, t, TOTAL_260, CHAIN_260, settings), want, (fmt, settings))


# ---- case 3: aligned tiles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,kinds", [(3, [0, 2]), (2, [0])])
@pytest.mark.parametrize("fmt", FMTS)
def test_regions_whose_stream_bases_are_on_128_byte_lines(lib, dev, oracle, fmt, count, kinds):
    total = 8192
    regions = [(4096, 128, 128), (5120, 64, 64), (5376, 36, 8)][:count]
    settings = default_settings(fmt)
    first, end = regions[0][0], region_end(regions[-1])
    assert end - first == (1298 if count == 3 else 1280)
    # (a guarded payload sits on a 256-byte address) aligned tiles, with three regions an edge launch behind them
    assert planned_kinds(lib, fmt, settings, 256, total, first, end - first) == kinds
    x, t = reference(oracle, fmt, total, settings)
    assert_all_equal(run_regions(lib, dev, fmt, t, total, regions, settings), wanted(oracle, fmt, total, regions), (fmt, count))
    assert_all_equal(run_regions(lib, dev, fmt, x, total, regions), wanted(oracle, fmt, total, regions), (fmt, count, "plain"))


# ---- case 4: more than sixteen regions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [30, PER_LAUNCH, PER_LAUNCH + 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_more_regions_than_one_launch_takes(lib, dev, oracle, fmt, count):
    total = 6 * 341
    regions = CUBE[:count]
    settings = default_settings(fmt)
    x, t = reference(oracle, fmt, total, settings)
    want = wanted(oracle, fmt, total, regions)
    assert_all_equal(run_regions(lib, dev, fmt, t, total, regions, settings), want, (fmt, count))
    assert_all_equal(run_regions(lib, dev, fmt, x, total, regions), want, (fmt, count, "plain"))


# ---- case 5: gaps and empty regions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_gaps_and_empty_regions(lib, dev, oracle, fmt):
    settings = default_settings(fmt)
    x, t = reference(oracle, fmt, TOTAL_256, settings)
    assert [blocks_of(w, h) for _, w, h in GAPS] == [4096, 0, 256, 0, 4]
    pitches = [max(BPP[fmt] * w, 16) for _, w, _ in GAPS]       # (an empty region's output is no bytes between two guards)
    want = wanted(oracle, fmt, TOTAL_256, GAPS, pitches)
    assert_all_equal(run_regions(lib, dev, fmt, t, TOTAL_256, GAPS, settings, pitches), want, fmt)
    assert_all_equal(run_regions(lib, dev, fmt, x, TOTAL_256, GAPS, None, pitches), want, (fmt, "plain"))
    # the blocks between the regions were written nowhere: every output above sat between guards.  An empty list does nothing
    src = Guarded(dev, t.size, 0, t)
    assert lib.dxtlt_untransform_decode_images_device(FMT_ID[fmt], src.ptr, TOTAL_256, None, 0, settings[0], settings[1], settings[2],
                                                      None) == OK
    assert lib.dxtlt_decode_images_device(FMT_ID[fmt], src.ptr, TOTAL_256, None, 0, None) == OK
    assert lib.dxtlt_untransform_decode_images(FMT_ID[fmt], t.ctypes.data, t.size, None, 0, settings[0], settings[1], settings[2]) == OK


# ---- case 6: the store policy is per region ----------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", [0, 1, 8])
@pytest.mark.parametrize("fmt", FMTS)
def test_every_region_has_a_store_policy_of_its_own(lib, dev, oracle, fmt, in_off):
    bpp = BPP[fmt]
    settings = default_settings(fmt)
    regions = CHAIN_260
    row = [bpp * w for _, w, _ in regions]
    pitches, offs = list(row), [0] * len(regions)
    pitches[0] = (row[0] + 15) // 16 * 16                    # level 0: the pixel pointer and the pitch multiples of 16 -- streaming stores
    pitches[1] = row[1] + 20                                 # level 1: a pitch that is no multiple of 16 -- plain stores
    offs[2], offs[3], offs[4] = 4, 8, 12                     # levels 2, 3, 4: pixel pointers at 4, 8, 12 from a 16-byte address
    if fmt == "bc4":                                         # an odd address with an odd pitch: byte stores
        offs[5], pitches[5] = 3, row[5] + 3
        assert (GUARD + offs[5]) % 2 == 1 and pitches[5] % 2 == 1
    assert pitches[0] % 16 == 0 and pitches[1] % 16 != 0
    x, t = reference(oracle, fmt, TOTAL_260, settings)
    want = wanted(oracle, fmt, TOTAL_260, regions, pitches)
    assert_all_equal(run_regions(lib, dev, fmt, t, TOTAL_260, regions, settings, pitches, offs, in_off), want, (fmt, in_off))
    assert_all_equal(run_regions(lib, dev, fmt, x, TOTAL_260, regions, None, pitches, offs, in_off), want, (fmt, in_off, "plain"))


# ---- case 7: the three routes agree ------------------------------------------------------------------------------------
# three regions, the middle one empty, 9 pixels wide: rows of 9, 18 and 36 bytes, which the host call stages 16, 32 and 48 apart
NINE_WIDE, TOTAL_NINE = [(1000, 9, 50), (2**63, 0, 7), (1050, 9, 14)], 1100


@pytest.mark.parametrize("fmt", FMTS)
def test_fused_plain_and_host_calls_agree(lib, dev, oracle, fmt):
    settings = default_settings(fmt)
    for regions, total in ((CHAIN_260, TOTAL_260), (NINE_WIDE, TOTAL_NINE)):
        pitches = [BPP[fmt] * w + 20 for _, w, _ in regions]
        x, t = reference(oracle, fmt, total, settings)
        want = wanted(oracle, fmt, total, regions, pitches)
        fused = run_regions(lib, dev, fmt, t, total, regions, settings, pitches)
        plain = run_regions(lib, dev, fmt, x, total, regions, None, pitches)
        hosts = [np.full(GUARD + (pitches[i] * h if w and h else 0) + GUARD, 0xA5, dtype=np.uint8) for i, (_, w, h) in enumerate(regions)]
        src = np.full(GUARD + t.size + GUARD, 0xA5, dtype=np.uint8)
        src[GUARD:GUARD + t.size] = t
        arr = region_array(regions, [h.ctypes.data + GUARD for h in hosts], pitches)
        rc = lib.dxtlt_untransform_decode_images(FMT_ID[fmt], src.ctypes.data + GUARD, t.size, arr, len(regions), settings[0], settings[1],
                                                 settings[2])
        assert rc == OK
        assert np.array_equal(src[GUARD:GUARD + t.size], t) and (src[:GUARD] == 0xA5).all() and (src[GUARD + t.size:] == 0xA5).all()
        host = []
        for i, h in enumerate(hosts):
            assert (h[:GUARD] == 0xA5).all() and (h[len(h) - GUARD:] == 0xA5).all(), "guard bytes were written"
            host.append(h[GUARD:len(h) - GUARD])
        assert_all_equal(fused, want, ("fused", total))
        assert_all_equal(plain, want, ("plain", total))
        assert_all_equal(host, want, ("host", total))


# ---- case 8: graph capture ---------------------------------------------------------------------------------------------
def test_fused_call_replays_from_a_hip_graph(lib, dev, oracle):
    import torch

    fmt, regions, total = "bc3", CHAIN_256, TOTAL_256
    settings = default_settings(fmt)
    x, t = reference(oracle, fmt, total, settings)
    pitches = default_pitches(fmt, regions)
    src = Guarded(dev, t.size, 0, t)
    dst = outputs(dev, regions, pitches)

    def work():
        # the table lives for the length of the call only: it is frozen into the captured launches
        arr = region_array(regions, [d.ptr for d in dst], pitches)
        rc = lib.dxtlt_untransform_decode_images_device(FMT_ID[fmt], src.ptr, total, arr, len(regions), settings[0], settings[1],
                                                        settings[2], torch.cuda.current_stream(dev).cuda_stream)
        assert rc == OK

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        work()                                    # warm-up outside capture (module load, first launch)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    # new blocks in the same buffer, the outputs cleared: only a replay can produce the right images now
    x2, t2 = reference(oracle, fmt, total, settings, seed=1)
    assert not np.array_equal(x, x2)
    src.view.copy_(torch.from_numpy(t2.copy()).to(dev))
    for d in dst:
        d.view.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert_all_equal([d.bytes() for d in dst], wanted(oracle, fmt, total, regions, seed=1), "replay")
    assert np.array_equal(src.bytes(), t2)


# ---- case 9: Python ----------------------------------------------------------------------------------------------------
def test_python_module_on_tensors_and_host_buffers(pkg, dev, oracle):
    import torch

    from dxt_lossless_transform_amd import image

    regions, total = image.mip_chain(260, 136, 9)
    assert (regions, total) == (CHAIN_260, TOTAL_260)
    for k, (first, w, h) in enumerate(regions):
        lw, lh, lfirst, num, ltotal = image.mip_level(260, 136, 9, k)
        assert (first, w, h, total) == (lfirst, lw, lh, ltotal) and num == blocks_of(w, h)
    for fmt in FMTS:
        settings = default_settings(fmt)
        x, t = reference(oracle, fmt, total, settings)
        want = [image_of(oracle, fmt, total, r).reshape(-1) for r in regions]
        if fmt in ("bc4", "bc5"):
            kw = dict(split_endpoints=settings[1])
        else:
            kw = dict(decorrelation_mode=pkg.YCoCgVariant.Variant1, split_alpha_endpoints=True, split_colour_endpoints=True)
        got = image.untransform_decode_images(fmt, torch.from_numpy(t.copy()).to(dev), regions, **kw)
        torch.cuda.synchronize()
        assert_all_equal([g.cpu().numpy() for g in got], want, (fmt, "tensors"))
        assert_all_equal(image.untransform_decode_images(fmt, t, regions, **kw), want, (fmt, "host buffers"))
        got = image.decode_images(fmt, torch.from_numpy(x.copy()).to(dev), regions)
        torch.cuda.synchronize()
        assert_all_equal([g.cpu().numpy() for g in got], want, (fmt, "plain"))
        # caller's outputs and pitches; a sub-list of the regions and total_blocks given
        pitches = [BPP[fmt] * w + 4 for _, w, _ in regions[1:4]]
        outs = [np.full(p * h, 0xA5, np.uint8) for p, (_, _, h) in zip(pitches, regions[1:4])]
        back = image.untransform_decode_images(fmt, t, regions[1:4], total_blocks=total, outs=outs, pitches=pitches, **kw)
        assert all(a is b for a, b in zip(back, outs))
        for i, r in enumerate(regions[1:4]):
            assert np.array_equal(outs[i], expected_buffer(image_of(oracle, fmt, total, r), pitches[i]))
    with pytest.raises(TypeError):
        image.decode_images("bc1", x, regions)
