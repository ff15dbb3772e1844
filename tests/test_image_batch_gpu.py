"""The images of many transformed buffers in one call on the MI355X (include/dxtlt_image.h:
dxtlt_untransform_decode_images_batch_device).  Every image of every batch is compared byte for byte with the CPU statement -- the
oracle's decoder rearranged into rows, the oracle's transform for the input -- and with what
dxtlt_untransform_decode_images_device writes for the same item alone.  Every source and every output sits inside 0xA5 guards and
every output is prefilled with 0xA5: the guards, the pitch padding and the bytes behind each image's last row must still be 0xA5
afterwards, and no source changes.  The batches are tests/image_batch_common.py's; tests/test_image_batch_layout.py proves on the
host which tile forms and lookup paths they reach.  The largest image is 260 pixels wide."""
import numpy as np
import pytest

from image_batch_common import GPU_BATCHES, batch_items, item_out_offs, item_pitches, load
from image_regions_common import (BPP, CHAIN_256, CHAIN_260, FMT_ID, FMTS, OK, TOTAL_256, TOTAL_260, Guarded, default_settings,
                                  expected_buffer, image_of, reference, region_array)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(pkg):
    return load(pkg)


def outputs_of(dev, it):
    pitches, offs = item_pitches(it), item_out_offs(it)
    return [Guarded(dev, pitches[k] * h if w and h else 0, offs[k]) for k, (_, w, h) in enumerate(it.regions)]


def run_batch(lib, dev, oracle, items):
    """the batch in ONE call and every item through the single call, both checked against the CPU statement"""
    import torch

    sources, src_of = {}, []
    for i, it in enumerate(items):
        key = ("shared", it.share) if it.share is not None else i
        if key not in sources:
            t = reference(oracle, it.fmt, it.total, it.settings, it.seed)[1] if it.regions else np.zeros(0, np.uint8)
            sources[key] = (Guarded(dev, t.size, it.in_off, t), t)
        src_of.append(sources[key][0])
    batch_out = [outputs_of(dev, it) for it in items]
    single_out = [outputs_of(dev, it) for it in items]
    keep = []
    arr = batch_items(items, [s.ptr for s in src_of], [[d.ptr for d in outs] for outs in batch_out], keep)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        assert lib.dxtlt_untransform_decode_images_batch_device(arr, len(items), stream) == OK, lib.dxtlt_last_error()
        for i, it in enumerate(items):
            regs = region_array(it.regions, [d.ptr for d in single_out[i]], item_pitches(it))
            assert lib.dxtlt_untransform_decode_images_device(FMT_ID[it.fmt], src_of[i].ptr, it.total, regs, len(it.regions),
                                                              it.settings[0], it.settings[1], it.settings[2], stream) == OK
    torch.cuda.synchronize()
    for guarded, t in sources.values():
        assert np.array_equal(guarded.bytes(), t), "a source buffer changed"
    images = 0
    for i, it in enumerate(items):
        pitches = item_pitches(it)
        for k, region in enumerate(it.regions):
            got = batch_out[i][k].bytes()   # (checks the guards)
            if region[1] == 0 or region[2] == 0:
                assert got.size == 0
                continue
            want = expected_buffer(image_of(oracle, it.fmt, it.total, region, it.seed), pitches[k])
            assert np.array_equal(got, want), ("the CPU statement differs", i, it.fmt, it.settings, k, region)
            assert np.array_equal(got, single_out[i][k].bytes()), ("the single call differs", i, it.fmt, it.settings, k, region)
            images += 1
    return images


def test_mixed_batch(lib, dev, oracle):
    # ten (format, settings) launches whose items are scattered over the list, two items without an image in the middle
    assert run_batch(lib, dev, oracle, GPU_BATCHES["mixed"]()) == 10 * (9 + 9 + 1 + 1)


def test_every_setting_of_every_format_in_one_call(lib, dev, oracle):
    items = GPU_BATCHES["every setting"]()
    assert len(items) == 36
    assert run_batch(lib, dev, oracle, items) == 36 * 9


def test_aligned_and_shifted_ranges_in_one_launch(lib, dev, oracle):
    assert run_batch(lib, dev, oracle, GPU_BATCHES["aligned"]()) == 5 * (3 + 9 + 2)


def test_many_small_items(lib, dev, oracle):
    # 300 one-workgroup items and three chains per launch: the wide index, the bisection, rotated and unrotated entries
    items = GPU_BATCHES["many small"]()
    assert len(items) == 2 * 303
    assert run_batch(lib, dev, oracle, items) == 2 * (300 + 3 * 9)


def test_items_of_more_than_one_entry(lib, dev, oracle):
    assert run_batch(lib, dev, oracle, GPU_BATCHES["multi entry"]()) == 5 * (17 + 33 + 30)


def test_gaps_and_empty_regions(lib, dev, oracle):
    assert run_batch(lib, dev, oracle, GPU_BATCHES["gaps"]()) == 5 * 3


def test_items_sharing_a_buffer(lib, dev, oracle):
    assert run_batch(lib, dev, oracle, GPU_BATCHES["shared buffer"]()) == 5 * 9


def test_store_policy_per_region(lib, dev, oracle):
    assert run_batch(lib, dev, oracle, GPU_BATCHES["store policy"]()) == 5 * 3 * 9


def test_item_at_an_odd_address_between_two_ordinary_ones(lib, dev, oracle):
    assert run_batch(lib, dev, oracle, GPU_BATCHES["fallback"]()) == 5 * 3 * 9


def test_python_module_on_tensors_and_a_side_stream(pkg, dev, oracle):
    import torch

    from dxt_lossless_transform_amd import image

    items, want = [], []
    for fmt in FMTS:
        settings = default_settings(fmt)
        if fmt in ("bc4", "bc5"):
            kw = dict(split_endpoints=settings[1])
        else:
            kw = dict(decorrelation_mode=pkg.YCoCgVariant.Variant1, split_alpha_endpoints=True, split_colour_endpoints=True)
        for regions, total in ((CHAIN_256, TOTAL_256), (CHAIN_260, TOTAL_260)):
            t = reference(oracle, fmt, total, settings)[1]
            items.append((fmt, torch.from_numpy(t.copy()).to(dev), regions, kw))
            want.append([image_of(oracle, fmt, total, r).reshape(-1) for r in regions])
    got = image.untransform_decode_images_batch(items)
    torch.cuda.synchronize()
    assert [len(g) for g in got] == [9] * 10
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert np.array_equal(a.cpu().numpy(), b)
    # the caller's outputs and pitches, total_blocks given, on a side stream as torch's current stream
    fmt, regions = "bc3", CHAIN_260[1:4]
    pitches = [BPP[fmt] * w + 4 for _, w, _ in regions]
    outs = [torch.full((p * h,), 0xA5, dtype=torch.uint8, device=dev) for p, (_, _, h) in zip(pitches, regions)]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        back = image.untransform_decode_images_batch([("bc1", items[0][1], CHAIN_256[:2], items[0][3]),
                                                      (fmt, items[5][1], regions, dict(items[5][3], total_blocks=TOTAL_260, outs=outs,
                                                                                       pitches=pitches))])
    side.synchronize()
    assert all(a is b for a, b in zip(back[1], outs))
    for k, r in enumerate(regions):
        assert np.array_equal(outs[k].cpu().numpy(), expected_buffer(image_of(oracle, fmt, TOTAL_260, r), pitches[k]))
    for k, r in enumerate(CHAIN_256[:2]):
        assert np.array_equal(back[0][k].cpu().numpy(), image_of(oracle, "bc1", TOTAL_256, r).reshape(-1))
    assert image.untransform_decode_images_batch([]) == []
    with pytest.raises(TypeError):
        image.untransform_decode_images_batch([("bc1", reference(oracle, "bc1", TOTAL_256, default_settings("bc1"))[1], CHAIN_256)])
