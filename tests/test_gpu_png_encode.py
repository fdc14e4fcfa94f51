"""The device PNG encoder (csrc/png_encode.hip, include/hipac_png.h) against its restatement (tests/png_encode_cpu.py), byte
for byte, on the shared cases (tests/png_cases.py); guard bytes; determinism; argument checks; --write_png end to end."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as cases
import png_encode_cpu as ref
from ss25_hierarchical_multiscale_image_classification_amd import extract, png_encode as pe
from ss25_hierarchical_multiscale_image_classification_amd.patch_dataset import PatchDataset

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5
PAD = 11  # pixels of row padding: pitch_bytes > 3 W


@pytest.fixture(scope="module")
def dev_level():
    lv = cases.level()
    buf = torch.full((cases.H, cases.W + PAD, 3), 77, dtype=torch.uint8, device="cuda")
    buf[:, :cases.W] = torch.from_numpy(np.array(lv)).cuda()
    return buf


@pytest.fixture(scope="module")
def ref_files():
    lv = cases.level()
    return {(P, name): ref.encode_file(lv, *cases.CALLS[P][name], P) for P, name in cases.ALL_WINDOWS}


def guarded_call(level, xy, P, stride=None, *, W=cases.W, H=cases.H, n=None, ws_bytes=None, ws_shift=0):
    """One hipac_png_encode_windows call on buffers filled with FILL and followed by guards.  Returns (rc, files or None,
    whether every byte the call had no business writing still holds FILL)."""
    lib = pe.load_png_library()
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    n_real = len(xy)
    n = n_real if n is None else n
    stride = pe.out_stride(P) if stride is None else stride
    need = int(lib.hipac_png_workspace_bytes(P, n_real))
    out = torch.full((n_real * max(stride, 1) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n_real + 8,), -7, dtype=torch.int64, device="cuda")
    ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    xy_dev = torch.from_numpy(xy).cuda()
    rc = lib.hipac_png_encode_windows(level.data_ptr(), W, H, int(level.stride(0)), xy_dev.data_ptr(), n, P, out.data_ptr(), stride,
                                      sizes.data_ptr(), ws.data_ptr() + ws_shift, need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    out_h, sizes_h, ws_tail = out.cpu().numpy(), sizes.cpu().numpy(), ws[need:].cpu().numpy()
    intact = bool((ws_tail == FILL).all() and (sizes_h[n_real:] == -7).all() and (out_h[n_real * stride:] == FILL).all())
    if rc != 0:
        intact = intact and bool((out_h == FILL).all() and (sizes_h == -7).all() and (ws.cpu().numpy() == FILL).all())
        return rc, None, intact
    files = []
    for i in range(n_real):
        s = int(sizes_h[i])
        assert 0 < s <= ref.file_bound(P) <= stride
        files.append(out_h[i * stride:i * stride + s].tobytes())
        intact = intact and bool((out_h[i * stride + s:(i + 1) * stride] == FILL).all())
    return rc, files, intact


@pytest.mark.parametrize("P", sorted(cases.CALLS))
def test_device_files_equal_the_restatement(dev_level, ref_files, P):
    names = list(cases.CALLS[P])
    xy = [cases.CALLS[P][k] for k in names]
    rc, files, intact = guarded_call(dev_level, xy, P)
    assert rc == 0 and intact
    for name, f in zip(names, files):
        want = ref_files[P, name]
        assert len(f) == len(want), (P, name, len(f), len(want))
        assert f == want, (P, name, next(i for i in range(len(f)) if f[i] != want[i]))
    # a second run, and the windows in reverse order: the same bytes per window
    assert guarded_call(dev_level, xy, P)[1] == files
    assert guarded_call(dev_level, xy[::-1], P)[1] == files[::-1]
    # an unpadded stride (the bound itself) and a single window per call
    assert guarded_call(dev_level, xy[:2], P, stride=ref.file_bound(P))[1:] == (files[:2], True)
    assert guarded_call(dev_level, xy[-1:], P)[1:] == (files[-1:], True)


def test_encode_windows_binding_and_batches(dev_level, ref_files, monkeypatch):
    P = 86
    names = list(cases.CALLS[P])
    xy = np.array([cases.CALLS[P][k] for k in names], np.int32)
    buf, sizes = pe.encode_windows(dev_level, cases.W, cases.H, xy, P)
    stride = buf.numel() // len(names)
    assert sizes.dtype == torch.int64 and sizes.is_cuda and buf.dtype == torch.uint8 and stride == pe.out_stride(P)
    host, sz = buf.cpu().numpy(), sizes.cpu().numpy()
    for i, name in enumerate(names):
        assert host[i * stride:i * stride + sz[i]].tobytes() == ref_files[P, name]
    # batches of three windows: the same files, in order
    got = {}
    for lo, files in pe.iter_encoded(dev_level, cases.W, cases.H, xy, P, budget=3 * pe.out_stride(P)):
        assert len(files) <= 3
        for k, f in enumerate(files):
            got[lo + k] = f
    assert [got[i] for i in range(len(names))] == [ref_files[P, k] for k in names]
    f = got[0]
    im = Image.open(io.BytesIO(f))
    im.load()
    assert np.array_equal(np.asarray(im), ref.window_pixels(cases.level(), *cases.CALLS[P][names[0]], P))


def test_bad_arguments_launch_nothing(dev_level, ref_files):
    P = 5
    names = list(cases.CALLS[P])
    xy = [cases.CALLS[P][k] for k in names]
    need = pe.load_png_library().hipac_png_workspace_bytes(P, len(xy))
    for kw, code in ((dict(W=0), -1), (dict(H=-1), -1), (dict(n=0), -1), (dict(n=pe.PNG_MAX_WINDOWS + 1), -1),
                     (dict(ws_bytes=need - 1), -2), (dict(ws_shift=8), -1), (dict(stride=ref.file_bound(P) - 1), -1),
                     (dict(W=cases.W + PAD + 1), -1)):  # 3 W above the pitch
        rc, files, intact = guarded_call(dev_level, xy, P, **kw)
        assert rc == code and files is None and intact, kw
    rc, _, intact = guarded_call(dev_level, xy, 1793, stride=4096)
    assert rc == -1 and intact
    rc, files, intact = guarded_call(dev_level, xy, P)
    assert rc == 0 and intact and files == [ref_files[P, k] for k in names]


def test_write_png_device_equals_host_tree(tmp_path):
    """A small synthetic slide whose level 3 is 700 x 500: border windows, dropped white windows, both encoders."""
    slide = extract.DeviceSlide.synthetic(5600, 4000, seed=12, name="tumor_012")
    level = 3
    assert slide.level_dimensions[level] == (700, 500)
    scan = extract.scan_level(slide, level)
    keep = scan.keep.cpu().numpy().astype(bool)
    xy = scan.xy.cpu().numpy()
    assert scan.patch_size == 224 and 0 < keep.sum() < len(keep)  # at least one window dropped as white
    assert any(x + 224 > 700 or y + 224 > 500 for (x, y), k in zip(xy, keep) if k)  # a kept border window
    host_dir, dev_dir = tmp_path / "host", tmp_path / "device"
    n_host = extract.save_patch_pngs(slide, level, str(host_dir))
    # a file that already exists is left alone, and counted
    first = sorted(os.listdir(host_dir / slide.name))[0]
    os.makedirs(dev_dir / slide.name)
    (dev_dir / slide.name / first).write_bytes(b"kept as it is")
    n_dev = extract.save_patch_pngs(slide, level, str(dev_dir), encoder="device")
    assert n_dev == n_host == int(keep.sum())
    names = sorted(os.listdir(host_dir / slide.name))
    assert names == sorted(os.listdir(dev_dir / slide.name))
    assert (dev_dir / slide.name / first).read_bytes() == b"kept as it is"
    os.remove(dev_dir / slide.name / first)
    assert extract.save_patch_pngs(slide, level, str(dev_dir), encoder="device") == n_host  # only the missing file is written
    for name in names:
        a, b = Image.open(host_dir / slide.name / name), Image.open(dev_dir / slide.name / name)
        a.load(), b.load()
        assert b.mode == "RGB" and np.array_equal(np.asarray(a), np.asarray(b)), name
    ds_host = PatchDataset(str(host_dir), raw=True, verbose=False)
    ds_dev = PatchDataset(str(dev_dir), raw=True, verbose=False)
    lab = lambda ds: sorted((os.path.basename(p), l) for p, l in zip(ds.image_paths, ds.labels))
    assert lab(ds_host) == lab(ds_dev) and len(ds_dev) == n_host
    img, label, path = ds_dev[0]
    assert tuple(img.shape) == (224, 224, 3) and label in (0, 1)
    with pytest.raises(Exception):
        extract.save_patch_pngs(slide, level, str(dev_dir), encoder="gpu")
