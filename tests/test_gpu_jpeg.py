"""JPEG tiles of a tiled pyramidal TIFF decoded on the device (csrc/jpeg_decode.hip) against the host decoder -- Pillow's
libjpeg, the arithmetic openslide reaches for the reference (src/main.py:650, :693): bit for bit, for every tile layout the
device decoder takes, and with the host fallback for the ones it does not."""
import numpy as np
import pytest
import torch

import jpeg_cases
from ss25_hierarchical_multiscale_image_classification_amd import extract, synth, tiff_pyramid

pytestmark = pytest.mark.gpu


def _pyramid(w, h, seed, noise=False):
    if noise:
        l0 = torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    else:
        l0 = synth.synth_level0(w, h, seed=seed, device="cpu")
    return [t.numpy() for t in synth.build_pyramid(l0, 3)]


def _both(path, workers=4):
    tp = tiff_pyramid.TiffPyramid(path)
    dev = [t.cpu() for t, _ in tp.to_device_levels("cuda", workers=workers)]
    host = [t.cpu() for t, _ in tiff_pyramid.TiffPyramid(path).to_device_levels("cuda", workers=workers, device_jpeg=False)]
    return tp, dev, host


@pytest.mark.parametrize("tile,quality,tables,sub,bigtiff,noise", [
    (256, 90, False, -1, False, False), (512, 75, True, -1, True, False), (256, 30, True, -1, False, False),
    (256, 100, False, -1, False, True), (128, 95, True, 0, False, False), (256, 100, False, 0, False, True),
    (64, 85, False, -1, False, False), (48, 85, False, -1, False, False), (256, 80, True, 1, False, False), (128, 100, False, 1, True, True)])
def test_device_jpeg_equals_the_host_decoder(tmp_path, tile, quality, tables, sub, bigtiff, noise):
    levels = _pyramid(1500, 1100, 3 + tile + quality, noise)
    path = str(tmp_path / "s.tif")
    tiff_pyramid.write_tiled_tiff(path, levels, tile=tile, compression="jpeg", quality=quality, jpeg_tables=tables, subsampling=sub,
                                  bigtiff=bigtiff)
    tp, dev, host = _both(path)
    n_tiles = sum(l.tiles_across * l.tiles_down for l in tp.levels)
    assert tp.device_decoded == n_tiles  # every tile went through the device decoder
    for a, b in zip(dev, host):
        assert torch.equal(a, b), int((a != b).sum())


def test_restart_markers_optimised_tables_and_fallbacks(tmp_path):
    levels = _pyramid(900, 700, 8)
    cases = [({"restart_marker_rows": 1}, -1, True), ({"restart_marker_blocks": 5}, 0, True), ({"optimize": True}, -1, True),
             ({"progressive": True}, -1, False)]  # progressive tiles: the host decodes them
    for k, (opts, sub, on_device) in enumerate(cases):
        path = str(tmp_path / f"s{k}.tif")
        tiff_pyramid.write_tiled_tiff(path, levels, tile=256, compression="jpeg", quality=88, subsampling=sub, jpeg_options=opts)
        tp, dev, host = _both(path)
        n_tiles = sum(l.tiles_across * l.tiles_down for l in tp.levels)
        if on_device:
            assert tp.device_decoded == n_tiles, (opts, tp.device_decoded)  # optimised tables too: 17 tiles, 17 table sets, 64 planned for
        else:
            assert getattr(tp, "device_decoded", 0) == 0, opts
        for a, b in zip(dev, host):
            assert torch.equal(a, b), (opts, sub, int((a != b).sum()))
    # optimised tables in more tiles than a call plans configurations for: the tiles of the first 64 distinct configurations
    # (counted as tests/jpeg_cases.py counts them) are decoded on the device, exactly the others on the host
    path = str(tmp_path / "many.tif")
    tiff_pyramid.write_tiled_tiff(path, levels, tile=64, compression="jpeg", quality=88, jpeg_options={"optimize": True})
    tp = tiff_pyramid.TiffPyramid(path)
    on_host, decode_tile = [], tp._decode_tile
    tp._decode_tile = lambda lv, i: (on_host.append((tp.levels.index(lv), i)), decode_tile(lv, i))[1]
    dev = [t.cpu() for t, _ in tp.to_device_levels("cuda", workers=4)]
    host = [t.cpu() for t, _ in tiff_pyramid.TiffPyramid(path).to_device_levels("cuda", workers=4, device_jpeg=False)]
    flat = [(li, i) for li, lv in enumerate(tp.levels) for i in range(lv.tiles_across * lv.tiles_down)]
    raw = {k: bytes(tp._buf[tp.levels[k[0]].offsets[k[1]]:tp.levels[k[0]].offsets[k[1]] + tp.levels[k[0]].counts[k[1]]]) for k in flat}
    ok = jpeg_cases.within_config_limit([jpeg_cases.Level(lv.width, lv.height, 64, 64) for lv in tp.levels],
                                        [jpeg_cases.Tile(raw[k], 0, 0, k[0]) for k in flat])
    assert len(flat) == 165 + 48 + 12 and not ok.all()
    assert tp.device_decoded + len(on_host) == len(flat) and tp.device_decoded >= 64
    assert sorted(on_host) == [k for k, v in zip(flat, ok) if not v]
    for a, b in zip(dev, host):
        assert torch.equal(a, b), int((a != b).sum())


def test_missing_tiles_and_the_slide_object(tmp_path):
    levels = _pyramid(1300, 1000, 12)
    path = str(tmp_path / "s.tif")
    tiff_pyramid.write_tiled_tiff(path, levels, tile=256, compression="jpeg", quality=90, jpeg_tables=True, missing=[(0, 1, 2), (1, 0, 0)])
    tp, dev, host = _both(path)
    assert all(torch.equal(a, b) for a, b in zip(dev, host))
    assert not dev[0][256:512, 512:768].any()  # the missing tile stays zero
    slide = extract.DeviceSlide.from_tiff(path, n_levels=3)
    for lv, ref in zip(slide.levels, host):
        assert torch.equal(lv.cpu(), ref)


def test_corrupt_entropy_data_is_contained(tmp_path):
    """Bit flips and truncation inside the entropy-coded segments: every lane's walk still ends (zeros are fed behind a short
    or broken stream, as libjpeg does), nothing is written outside the tile's own scratch, and the tiles that were not touched
    decode exactly as before."""
    levels = _pyramid(1300, 1100, 17)
    clean = str(tmp_path / "clean.tif")
    tiff_pyramid.write_tiled_tiff(clean, levels, tile=256, compression="jpeg", quality=85, jpeg_tables=True)
    ref = [t.cpu() for t, _ in tiff_pyramid.TiffPyramid(clean).to_device_levels("cuda", device_jpeg=False)]
    data = bytearray(open(clean, "rb").read())
    tp = tiff_pyramid.TiffPyramid(clean)
    rng = np.random.default_rng(5)
    lv0 = tp.levels[0]
    n = lv0.tiles_across * lv0.tiles_down
    hit = sorted(rng.choice(n, 6, replace=False).tolist())
    for k, i in enumerate(hit):
        off, cnt = lv0.offsets[i], lv0.counts[i]
        if k % 3 == 0:  # random bit flips behind the (short) tile header
            for _ in range(40):
                p = off + 60 + int(rng.integers(0, cnt - 62))
                data[p] ^= 1 << int(rng.integers(0, 8))
        elif k % 3 == 1:  # runs of 0xFF (markers / stuffing in the middle of the data)
            p = off + 80 + int(rng.integers(0, cnt // 2))
            data[p:p + 9] = b"\xff\x00\xff\xff\xd3\xff\xd9\xff\x17"
        else:  # the second half of the stream zeroed (a truncated write)
            data[off + cnt // 2:off + cnt] = bytes(cnt - cnt // 2)
    broken = str(tmp_path / "broken.tif")
    open(broken, "wb").write(bytes(data))
    tpb = tiff_pyramid.TiffPyramid(broken)
    got = [t.cpu() for t, _ in tpb.to_device_levels("cuda")]
    assert tpb.device_decoded == sum(l.tiles_across * l.tiles_down for l in tpb.levels)
    for li, (a, b) in enumerate(zip(got, ref)):
        if li > 0:
            assert torch.equal(a, b)
            continue
        same = torch.ones(n, dtype=torch.bool)
        for i in range(n):
            ty, tx = divmod(i, lv0.tiles_across)
            ya, xa = ty * 256, tx * 256
            same[i] = torch.equal(a[ya:ya + 256, xa:xa + 256], b[ya:ya + 256, xa:xa + 256])
        assert all(bool(same[i]) for i in range(n) if i not in hit)  # the damage stays inside the damaged tiles
