"""Generate tests/golden/froc_golden.npz: mask levels and their evaluation masks / ITC lists.

    python tests/golden/make_golden_froc.py

Source of truth: scipy's distance_transform_edt / binary_fill_holes / label through tests/froc_cpu.py (the pipeline of
the CAMELYON16 script, scikit-image's label(connectivity=2) being scipy's label with a 3x3 structure).  Every case is
(mask uint8[H, W], resolution, level); `resolution` other than 0.243 sets the distance threshold directly.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import froc_cpu  # noqa: E402


def disks(shape, centres_radii, hole=None):
    rr, cc = np.mgrid[:shape[0], :shape[1]]
    m = np.zeros(shape, np.uint8)
    for (r, c, rad) in centres_radii:
        m[(rr - r) ** 2 + (cc - c) ** 2 <= rad * rad] = 255
    return m


def res_for_threshold(t, level=5):  # resolution giving eval threshold t at `level`
    return 75 / (t * pow(2, level) * 2)


def cases():
    rng = np.random.default_rng(16)
    out = []
    # blobs with holes (ellipses with an elliptic hole, a few dots)
    rr, cc = np.mgrid[:300, :400]
    m = np.zeros((300, 400), np.uint8)
    for _ in range(7):
        r, c, a, b = rng.integers(30, 270), rng.integers(30, 370), rng.integers(12, 40), rng.integers(12, 40)
        e = ((rr - r) / a) ** 2 + ((cc - c) / b) ** 2
        m[(e <= 1) & (e > 0.35)] = 255
    m[rng.random((300, 400)) < 0.0008] = 255
    out.append(("blobs_with_holes", m, 0.243, 5))
    # a ring whose hole survives the 4.82-pixel dilation, and one whose hole is filled
    rr, cc = np.mgrid[:160, :200]
    d2 = (rr - 80) ** 2 + (cc - 60) ** 2
    m = np.zeros((160, 200), np.uint8)
    m[(d2 >= 30 ** 2) & (d2 <= 40 ** 2)] = 255
    d2 = (rr - 80) ** 2 + (cc - 160) ** 2
    m[(d2 >= 6 ** 2) & (d2 <= 14 ** 2)] = 255
    out.append(("ring", m, 0.243, 5))
    # threshold 0.9: binary == (mask == 255).  A hole whose only way out is a diagonal step (4-connectivity keeps it
    # a hole: filled), and two blobs that touch only at a corner (8-connectivity: one label)
    m = np.zeros((24, 30), np.uint8)
    m[2:9, 2:9] = 255
    m[3:8, 3:8] = 0
    m[2, 2] = 0
    m[12:16, 4:8] = 255
    m[16:20, 8:12] = 255
    m[14:22, 16] = 255
    m[13, 17] = 255
    out.append(("diagonal_leak", m, res_for_threshold(0.9), 5))
    # blobs touching all four borders (the background pockets between them and the border are not holes)
    m = disks((120, 150), [(0, 75, 20), (119, 40, 18), (60, 0, 25), (70, 149, 22), (60, 75, 10)])
    m[40:80, 60:62] = 0
    out.append(("touching_borders", m, 0.243, 5))
    # no byte == 255: scipy's virtual zero at (row -1, column 0)
    out.append(("empty", np.zeros((40, 50), np.uint8), 0.243, 5))
    out.append(("empty_level2", np.full((90, 120), 7, np.uint8), 0.243, 2))
    out.append(("all_255", np.full((30, 30), 255, np.uint8), 0.243, 5))
    # degenerate shapes
    m = np.zeros((1, 200), np.uint8)
    m[0, [5, 17, 60, 61, 150]] = 255
    out.append(("row_1xN", m, 0.243, 5))
    m = np.zeros((200, 1), np.uint8)
    m[[0, 33, 120, 199], 0] = 255
    out.append(("col_Nx1", m, 0.243, 5))
    m = (rng.random((257, 263)) < 0.004).astype(np.uint8) * 255
    m[100:140, 30:90] = 255
    out.append(("odd_257x263", m, 0.243, 5))
    # ITC: discs whose evaluation region's major axis straddles 35.36 pixels, and thin ellipses
    rr, cc = np.mgrid[:200, :260]
    m = disks((200, 260), [(30, 30, 11), (30, 100, 12), (30, 170, 13), (30, 235, 14)])
    for (r, c, a, b) in [(110, 40, 2, 13), (110, 110, 3, 14), (110, 180, 1, 16), (170, 60, 5, 12), (170, 160, 7, 11)]:
        m[((rr - r) / a) ** 2 + ((cc - c) / b) ** 2 <= 1] = 255
    out.append(("itc_sizes", m, 0.243, 5))
    # large radii: level 0 (threshold 154 px) and level 2 (38.6 px)
    m = np.zeros((400, 420), np.uint8)
    m[[10, 200, 390], [15, 300, 100]] = 255
    m[180:190, 20:24] = 255
    out.append(("level0_dots", m, 0.243, 0))
    m = np.zeros((300, 330), np.uint8)
    m[rng.integers(0, 300, 12), rng.integers(0, 330, 12)] = 255
    out.append(("level2_dots", m, 0.243, 2))
    return out


def main():
    data = {}
    names = []
    for name, m, res, level in cases():
        labels = froc_cpu.evaluation_mask(m, res, level)
        axes = froc_cpu.major_axes(labels)
        thr = 275 / (res * pow(2, level))
        assert all(abs(a - thr) > 1e-6 * thr for a in axes), (name, axes)  # no ITC decision at rounding distance
        itc = froc_cpu.itc_list(labels, res, level)
        data[f"{name}__mask"] = m
        data[f"{name}__labels"] = labels
        data[f"{name}__params"] = np.array([res, level], np.float64)
        data[f"{name}__itc"] = np.asarray(itc, np.int32)
        names.append(name)
        print(f"{name}: {m.shape}, level {level}, {labels.max()} labels, ITC {itc}")
    data["names"] = np.array(names)
    path = os.path.join(HERE, "froc_golden.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
