"""LZW tiles decoded on the device (csrc/lzw.hip) against the host definition tiff_pyramid.lzw_decode, bit for bit: streams of
both encoders (ours and libtiff's) as single tiles, pyramids through to_device_levels, refused streams among valid neighbours,
read_mask_level, DeviceSlide.from_tiff and --run_evaluation."""
import json
import os

import numpy as np
import pytest
import torch

import lzw_cases
from ss25_hierarchical_multiscale_image_classification_amd import extract, tiff_pyramid as tp

pytestmark = pytest.mark.gpu


def rgb_of(a):
    """uint8[h, w, s] samples -> the RGB a level holds: 1 replicated, 3 as is, 4 without alpha."""
    return np.repeat(a, 3, 2) if a.shape[2] == 1 else a[:, :, :3]


def device_tiles(streams, rows, w, samples, predictor, across=1):
    """``streams`` side by side as the tiles of one level of ``across * w`` x ``rows``: (uint8[rows, pitch, 3], status)."""
    W = across * w
    dev = torch.full((rows, (W + 15) // 16 * 16, 3), 0, dtype=torch.uint8, device="cuda")
    off = np.cumsum([0] + [len(s) for s in streams[:-1]]).astype(np.int64)
    cnt = np.array([len(s) for s in streams], np.int64)
    xyl = np.array([[k * w, 0, 0] for k in range(len(streams))], np.int32)
    file_dev = torch.frombuffer(bytearray(b"".join(streams)), dtype=torch.uint8).cuda()  # no byte behind the last stream
    status = tp.device_lzw_tiles(file_dev, [(dev, W, rows, w, rows, samples, predictor)], off, cnt, xyl)
    return dev.cpu().numpy(), status


def check_single(stream, rows, w, samples, predictor):
    want, st = lzw_cases.host_decode(stream, rows, w, samples, predictor)
    got, status = device_tiles([stream], rows, w, samples, predictor)
    assert st == 0 and list(status) == [0]
    assert np.array_equal(got[:, :w], rgb_of(want))
    assert not got[:, w:].any()  # the padding columns of the 16-pixel pitch stay 0
    return want


@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("kind", lzw_cases.CONTENTS)
def test_streams_of_both_encoders_as_one_tile(kind, samples, predictor):
    h, w = 136, 200
    img = lzw_cases.content(kind, h, w, samples)
    stream, rows = lzw_cases.pillow_strips(img, predictor)[0]  # libtiff's stream: the first strip, a tile of the strip's shape
    want = check_single(stream, rows, w, samples, predictor)
    assert np.array_equal(want.reshape((rows,) + img.shape[1:]), img[:rows])
    raw = lzw_cases.difference(img) if predictor == 2 else img
    for clear_when_full in (True, False):  # ours, with and without the table-full Clear
        want = check_single(tp.lzw_encode(raw.tobytes(), clear_when_full), h, w, samples, predictor)
        assert np.array_equal(want.reshape(img.shape), img)


def test_a_large_random_tile_and_a_large_constant_tile():
    a = lzw_cases.content("random", 256, 256, 3)  # 192 KiB of output, some fifty Clears
    assert np.array_equal(check_single(tp.lzw_encode(a.tobytes()), 256, 256, 3, 1), a)
    c = lzw_cases.content("constant", 512, 512, 1)  # the longest strings, every code a KwKwK or an overlapping copy
    assert np.array_equal(check_single(tp.lzw_encode(c.tobytes()), 512, 512, 1, 1)[:, :, 0], c)
    assert np.array_equal(check_single(tp.lzw_encode(c.tobytes(), False), 512, 512, 1, 1)[:, :, 0], c)
    s = lzw_cases.pack9(256, 1, 2, 258, 256, 4, 4, 256, 256, 6, 257)  # three Clears, a short tile
    assert check_single(s, 1, 7, 1, 1).ravel().tolist() == [1, 2, 1, 2, 4, 4, 6]


def pyramid(samples):
    a = lzw_cases.content("random", 200, 300, samples)
    a[30:170, 40:260] = lzw_cases.content("gradient", 140, 220, samples)
    a[60:120, 100:200] = lzw_cases.content("blobs", 60, 100, samples)
    return [a, np.ascontiguousarray(a[::2, ::2]), np.ascontiguousarray(a[::4, ::4])]


@pytest.mark.parametrize("samples,predictor,bigtiff,missing", [(3, 1, False, ()), (3, 2, False, ()), (1, 2, False, ()), (4, 2, False, ()),
                                                                (4, 1, True, ()), (3, 2, True, ((0, 1, 2), (1, 0, 0))), (1, 1, False, ((0, 3, 4),))])
def test_pyramid_equals_the_host_path_bit_for_bit(tmp_path, samples, predictor, bigtiff, missing):
    levels = pyramid(samples)
    path = str(tmp_path / "s.tif")
    tp.write_tiled_tiff(path, levels, tile=64, compression="lzw", predictor=predictor, bigtiff=bigtiff, missing=missing)
    s = tp.TiffPyramid(path, samples=(1, 3, 4))
    dev = [t.cpu() for t, _ in s.to_device_levels("cuda")]
    again = [t.cpu() for t, _ in tp.TiffPyramid(path, samples=(1, 3, 4)).to_device_levels("cuda")]
    host = [t.cpu() for t, _ in tp.TiffPyramid(path, samples=(1, 3, 4)).to_device_levels("cuda", device_lzw=False)]
    n_tiles = sum(l.tiles_across * l.tiles_down for l in s.levels)
    assert s.device_decoded == n_tiles - len(missing)
    for k, (a, b, c) in enumerate(zip(dev, host, again)):
        assert a.shape == b.shape == (levels[k].shape[0], (levels[k].shape[1] + 15) // 16 * 16, 3)
        assert torch.equal(a, b), k  # the zero padding columns included
        assert torch.equal(a, c), k  # two runs give identical tensors
        if not missing:
            want = rgb_of(levels[k].reshape(levels[k].shape[0], levels[k].shape[1], -1))
            assert np.array_equal(a.numpy()[:, :levels[k].shape[1]], want)
        assert not a[:, levels[k].shape[1]:].any()


@pytest.mark.parametrize("case", ["truncated", "third code above the next free entry"])
def test_a_refused_or_truncated_tile_among_valid_neighbours(case):
    # the two malformed inputs the device sees: both end in the bounds checks of the parse, as a status
    tiles = [lzw_cases.content(k, 64, 64, 3) for k in ("random", "gradient", "blobs")]
    streams = [tp.lzw_encode(lzw_cases.difference(t).tobytes()) for t in tiles]
    streams[1] = streams[1][:len(streams[1]) // 2] if case == "truncated" else lzw_cases.REFUSED[case]
    want, st = lzw_cases.host_decode(streams[1], 64, 64, 3, 2)
    assert st == (0 if case == "truncated" else 1)
    got, status = device_tiles(streams, 64, 64, 3, 2, across=3)
    assert list(status) == [0, st, 0]
    assert np.array_equal(got[:, :64], tiles[0]) and np.array_equal(got[:, 128:192], tiles[2])
    assert np.array_equal(got[:, 64:128], want)
    if st:
        assert not got[:, 64:128].any()


def six_level_mask():
    full = lzw_cases.content("blobs", 1500, 1100, 1, seed=3)
    levels = [full]
    for _ in range(5):
        levels.append(np.ascontiguousarray(levels[-1][::2, ::2]))
    return levels


def test_read_mask_level_device_path_equals_host_path(tmp_path, monkeypatch):
    levels = six_level_mask()
    path = str(tmp_path / "tumor_001_Mask.tif")
    tp.write_tiled_tiff(path, levels, tile=256, compression="lzw", predictor=2)
    dev = {k: tp.read_mask_level(path, k) for k in (0, 5)}
    monkeypatch.setenv("HIPAC_DEVICE_LZW", "0")
    for k, a in dev.items():
        assert a.dtype == np.uint8 and np.array_equal(a, tp.read_mask_level(path, k)) and np.array_equal(a, levels[k])


def test_from_tiff_of_an_lzw_slide_scans_like_the_uncompressed_one(tmp_path):
    from ss25_hierarchical_multiscale_image_classification_amd import synth

    levels = [t.cpu().numpy() for t in synth.build_pyramid(synth.synth_level0(1200, 900, seed=4, device="cpu"), 3)]
    scans = []
    for name, kw in (("lzw", dict(compression="lzw", predictor=2)), ("none", dict(compression="none"))):
        path = str(tmp_path / f"{name}.tif")
        tp.write_tiled_tiff(path, levels, tile=256, **kw)
        slide = extract.DeviceSlide.from_tiff(path, n_levels=3)
        scans.append(extract.scan_level(slide, 1))
    assert torch.equal(scans[0].keep, scans[1].keep) and torch.equal(scans[0].sums, scans[1].sums)
    assert scans[0].keep.numel() > 0


def test_run_evaluation_takes_a_case_with_an_lzw_mask(tmp_path, monkeypatch, capsys):
    from ss25_hierarchical_multiscale_image_classification_amd import main

    levels = six_level_mask()
    root = tmp_path / "data"
    os.makedirs(root / "test" / "mask")
    out_dir = tmp_path / "models" / "first_model" / "model_predictions_csv"
    os.makedirs(out_dir)
    tp.write_tiled_tiff(str(root / "test" / "mask" / "tumor_001_Mask.tif"), levels, tile=128, compression="lzw")
    ys, xs = np.nonzero(levels[0])
    with open(out_dir / "tumor_001.csv", "w") as f:
        f.write(f"0.9,{xs[0]},{ys[0]}\n0.4,3,3\n")
    monkeypatch.chdir(tmp_path)
    assert main.main(["--run_evaluation", "--data_root", str(root)]) == 0
    assert "Could not read the mask" not in capsys.readouterr().out
    got = json.load(open(tmp_path / "froc_results.json"))
    assert [c["case"] for c in got["cases"]] == ["tumor_001.csv"] and got["cases"][0]["num_of_tumors"] >= 1
