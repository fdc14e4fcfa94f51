"""Host side of the FROC evaluation (froc.py) against a fresh restatement of the CAMELYON16 script (tests/froc_cpu.py):
the TP / FP bookkeeping given the labels under the detections, the FROC curve, the detection CSV round trip, grayscale
mask TIFFs and the CLI's missing-folder answers."""
import os

import numpy as np
import pytest
import torch

import froc_cpu
from ss25_hierarchical_multiscale_image_classification_amd import features, froc, main, tiff_pyramid

LEVEL = 5


def host_fp_tp(Y, X, P, is_tumor, labels, itc):
    max_label = int(labels.max(initial=0)) if is_tumor else 0
    hits = [froc_cpu.label_at(labels, x, y, LEVEL) for x, y in zip(X, Y)] if is_tumor else [0] * len(X)
    return froc.fp_tp_from_hits(hits, X, Y, P, is_tumor, max_label, itc)


def same_case(a, b):
    assert a[0] == b[0]
    assert a[1].dtype == b[1].dtype == np.float32 and np.array_equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3] and a[4] == b[4]


def label_maps():
    """(labels, ITC list, is_tumor) hand-made cases."""
    lab = np.zeros((40, 50), np.int32)
    lab[2:10, 3:20] = 1
    lab[12:14, 30:32] = 2  # ITC
    lab[20:35, 5:45] = 3
    lab[36:39, 48:50] = 4
    yield lab, [2], True
    yield lab, [], True
    yield lab, [1, 2, 3, 4], True  # zero tumours: every lesion is an ITC
    yield np.zeros((10, 10), np.int32), [], True  # an empty evaluation mask
    yield lab, [], False  # a normal case: every detection is an FP


def detections(rng, n, shape):
    X = [int(v) for v in rng.integers(-64, shape[1] * 2 ** LEVEL + 64, n)]
    Y = [int(v) for v in rng.integers(-64, shape[0] * 2 ** LEVEL + 64, n)]
    P = [round(float(v), 6) for v in rng.random(n)]
    return Y, X, P


def test_fp_tp_matches_restatement_on_random_detections():
    rng = np.random.default_rng(3)
    for lab, itc, is_tumor in label_maps():
        for n in (0, 1, 40, 400):
            Y, X, P = detections(rng, n, lab.shape)
            same_case(host_fp_tp(Y, X, P, is_tumor, lab, itc), froc_cpu.compute_fp_tp(Y, X, P, is_tumor, lab, itc, LEVEL))


def test_itc_hit_is_neither_tp_nor_fp_and_tp_slots_are_float32():
    lab = np.zeros((8, 8), np.int32)
    lab[1, 1], lab[5, 5] = 1, 2
    s = 2 ** LEVEL
    # two probabilities that differ in float64 but round to the same float32: the second is not "greater"
    p1 = 0.30000001
    p2 = float(np.nextafter(p1, 1.0))
    assert np.float32(p1) == np.float32(p2) and p2 > p1
    X, Y, P = [s + 3, s + 4, 5 * s, s + 1], [s + 2, s + 5, 5 * s, 7 * s], [p1, p2, 0.9, 0.2]
    got = host_fp_tp(Y, X, P, True, lab, [2])
    ref = froc_cpu.compute_fp_tp(Y, X, P, True, lab, [2], LEVEL)
    same_case(got, ref)
    fps, tps, k, det, fp_summary = got
    assert fps == [0.2] and k == 1 and tps[1] == 0  # the ITC hit (0.9) counts nowhere; its slot stays 0
    assert det == {"Label 1": [p1, s + 3, s + 2]}  # p2 does not beat float32(p1)
    assert fp_summary == {"FP 0": [0.2, s + 1, 7 * s]}


def test_froc_curve_matches_quadratic_restatement():
    rng = np.random.default_rng(5)
    for trial in range(12):
        cases = []
        for lab, itc, is_tumor in label_maps():
            Y, X, P = detections(rng, int(rng.integers(0, 120)), lab.shape)
            if trial % 3 == 0:  # ties between FP and TP values, and float32-rounding neighbours
                P = [float(np.float32(p)) if i % 2 else p for i, p in enumerate(P)]
            cases.append(froc_cpu.compute_fp_tp(Y, X, P, is_tumor, lab, itc, LEVEL))
        if trial == 1:
            cases = [c for c in cases if c[2] == 0]  # no tumour at all: nan sensitivity, as the reference
        names = [f"c{i}.csv" for i in range(len(cases))]
        data = (names, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
        fps, sens = froc.computeFROC(data)
        rfps, rsens = froc_cpu.compute_froc(*data)
        assert fps.dtype == rfps.dtype == np.float64
        np.testing.assert_array_equal(fps, rfps)
        np.testing.assert_array_equal(sens, rsens)
        if np.isfinite(sens).all():
            assert froc.froc_score(fps, sens) == froc_cpu.froc_score(rfps, rsens)


def test_froc_score_definition():
    fps = np.array([9.0, 3.0, 1.0, 0.5, 0.0])
    sens = np.array([0.9, 0.8, 0.6, 0.5, 0.0])
    # rates 1/4: 0.0 ; 1/2: 0.5 ; 1: 0.6 ; 2: 0.6 ; 4: 0.8 ; 8: 0.8
    assert froc.froc_score(fps, sens) == pytest.approx((0.0 + 0.5 + 0.6 + 0.6 + 0.8 + 0.8) / 6, abs=0)
    assert froc.froc_score(np.array([10.0, 9.0]), np.array([1.0, 0.5])) == 0.0


def test_csv_round_trip_through_save_froc_csv(tmp_path):
    rng = np.random.default_rng(7)
    n = 50
    logits = torch.from_numpy(rng.normal(size=(n, 2)).astype(np.float32))
    meta = np.stack([rng.integers(0, 4, n), rng.integers(0, 5000, n), rng.integers(0, 5000, n), rng.integers(0, 2, n)], 1)
    meta = torch.from_numpy(meta.astype(np.int32))
    ds = (1.0, 2.0, 4.0, 8.0)
    path = str(tmp_path / "tumor_009.csv")
    assert features.save_froc_csv(path, logits, meta, ds) == n
    probs, xs, ys = froc.readCSVContent(path)
    p = torch.softmax(logits, 1)[:, 1].numpy()
    assert probs == [float(f"{float(v):.6f}") for v in p]
    from ss25_hierarchical_multiscale_image_classification_amd.extract import PATCH_SIZES

    m = meta.numpy()
    assert xs == [int((x + PATCH_SIZES[l] / 2.0) * ds[l]) for l, x in zip(m[:, 0], m[:, 1])]
    assert ys == [int((y + PATCH_SIZES[l] / 2.0) * ds[l]) for l, y in zip(m[:, 0], m[:, 2])]
    assert all(isinstance(v, int) for v in xs + ys)


@pytest.mark.parametrize("compression", ["none", "deflate"])
def test_grayscale_mask_tiff_round_trip_at_level5(tmp_path, compression):
    rng = np.random.default_rng(11)
    H, W = 3000, 2100
    full = np.zeros((H, W), np.uint8)
    for _ in range(6):
        r, c, rad = rng.integers(0, H), rng.integers(0, W), rng.integers(20, 300)
        rr, cc = np.ogrid[:H, :W]
        full[(rr - r) ** 2 + (cc - c) ** 2 <= rad * rad] = 255
    levels = [full]
    for _ in range(6):
        levels.append(np.ascontiguousarray(levels[-1][::2, ::2]))
    path = str(tmp_path / "tumor_001_Mask.tif")
    tiff_pyramid.write_tiled_tiff(path, levels, tile=256, compression=compression)
    assert np.array_equal(tiff_pyramid.read_mask_level(path, 5), levels[5])
    with pytest.raises(tiff_pyramid.TiffError):
        tiff_pyramid.read_mask_level(path, 7)
    with pytest.raises(tiff_pyramid.TiffError):  # slides keep their 3 / 4-sample rule
        tiff_pyramid.TiffPyramid(path)
    from PIL import Image

    assert np.array_equal(np.asarray(Image.open(path)), full)  # a grayscale TIFF other readers take


def test_mask_sources_in_order(tmp_path):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "test", "mask", "annotations"))
    assert froc.mask_source(root, "test_001") is None
    xml = os.path.join(root, "test", "mask", "annotations", "test_001.xml")
    open(xml, "w").write("<ASAP_Annotations><Annotations></Annotations></ASAP_Annotations>")
    assert froc.mask_source(root, "test_001") == ("xml", xml)
    tif = os.path.join(root, "test", "mask", "test_001_Mask.tif")
    open(tif, "wb").close()
    assert froc.mask_source(root, "test_001") == ("tif", tif)


def test_run_evaluation_missing_folders_returns_1(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert main.main(["--run_evaluation"]) == 1
    out = capsys.readouterr().out
    mask_folder = os.path.join(str(tmp_path), "data", "camelyon16", "test", "mask")
    assert f"[ERROR] Evaluation mask folder '{mask_folder}' not found." in out
    os.makedirs(mask_folder)
    assert main.main(["--run_evaluation"]) == 1
    results = os.path.join(str(tmp_path), "models", "first_model", "model_predictions_csv")
    assert f"[ERROR] Model results folder '{results}' not found. Please run your detection model first." in capsys.readouterr().out


def test_run_evaluation_without_cases_warns(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    os.makedirs(tmp_path / "data" / "camelyon16" / "test" / "mask")
    os.makedirs(tmp_path / "models" / "first_model" / "model_predictions_csv")
    assert main.main(["--run_evaluation"]) == 0
    assert "No cases processed" in capsys.readouterr().out
    assert not (tmp_path / "froc_results.json").exists()
