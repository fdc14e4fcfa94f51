"""The scipy-free evaluation mask of tests/froc_cpu.py (`evaluation_mask_pure`) and the inputs of tests/froc_cases.py,
on the CPU: the restatement reproduces scipy's recorded labels of every golden case (and the live scipy pipeline where
scipy imports), and every case has the structure it was built for.  Integers throughout: every comparison is exact."""
import functools
import math
import os
import sys

import numpy as np
import pytest

import froc_cases
import froc_cpu

CASES = {name: (m, res, level) for name, m, res, level in froc_cases.cases()}


@functools.lru_cache(maxsize=None)
def pure(name):
    lab = froc_cpu.evaluation_mask_pure(*CASES[name])
    lab.setflags(write=False)
    return lab


def both(name):  # the T = 0.5 and T = 1.0 runs of a case (K = 1 in both)
    return [(CASES[f"{name}@{t}"][0], pure(f"{name}@{t}")) for t in (0.5, 1.0)]


def load_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "froc_golden.npz"))
    return [(str(n), z[f"{n}__mask"], z[f"{n}__labels"], float(z[f"{n}__params"][0]), int(z[f"{n}__params"][1]))
            for n in z["names"]]


def check_golden_pin(golden_dir):
    cases = load_golden(golden_dir)
    assert len(cases) == 13
    for name, mask, labels, res, level in cases:
        got = froc_cpu.evaluation_mask_pure(mask, res, level)
        assert got.dtype == np.int32 and np.array_equal(got, labels), name


def test_pure_reproduces_every_golden_label_image(golden_dir):
    check_golden_pin(golden_dir)


def test_threshold_k():
    k = lambda t: froc_cpu.threshold_k(froc_cases.res_for_threshold(t), froc_cases.LEVEL)
    assert [k(t) for t in (0.5, 1.0, 1.3, 1.5, 5.0)] == [1, 1, 2, 3, 25]
    assert k(math.nextafter(5.0, 6.0)) == 26
    for t in (0.5, 1.0, 5.0):  # these set the threshold exactly
        assert froc_cases.eval_threshold(froc_cases.res_for_threshold(t)) == t
    assert froc_cpu.threshold_k(0.243, 5) == 24 and froc_cpu.threshold_k(0.243, 0) == 23815
    for name, (m, res, level) in CASES.items():
        want = {"open_rings@1.3": 2, "pythagoras@5.0": 25, "pythagoras_next@5.0+": 26}.get(name, 1)
        assert froc_cpu.threshold_k(res, level) == want, name


def test_case_sizes():
    assert len(CASES) == 33
    for name, (m, _, _) in CASES.items():
        assert m.dtype == np.uint8 and m.size > froc_cases.CHUNK, name  # more than one numbering chunk (four workgroups)
        assert m.size <= 16384 or name.startswith("roots_on_chunks"), name


def check_structure():
    for m, lab in both("spiral_arm"):
        assert m.shape == (67, 71) and not m[:3].any() and not m[-3:].any() and not m[:, :3].any() and not m[:, -3:].any()
        assert lab.max() == 1 and (m == 255).sum() >= 1000
        assert np.array_equal(lab != 0, m == 255)  # nothing filled: the corridor is open to the border
        # the arm is a simple path, one pixel wide: two ends, every other pixel with exactly two 4-neighbours
        p = np.pad(m == 255, 1).astype(int)
        nb = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:])[m == 255]
        assert np.bincount(nb).tolist() == [0, 2, (m == 255).sum() - 2]
    for m, lab in both("open_rings"):
        assert lab.max() == 10 and np.array_equal(lab != 0, m == 255)
        assert np.unique(lab[31, :32]).tolist() == list(range(11))  # numbered from the outside in
    lab = pure("open_rings@1.3")
    assert lab.max() == 1 and (lab[1:-1, 1:-1] == 1).all() and (lab != 0).sum() > (CASES["open_rings@1.3"][0] == 255).sum()
    for m, lab in both("closed_rings"):
        assert lab.max() == 1 and (lab[1:-1, 1:-1] == 1).all()
        assert not lab[0].any() and not lab[-1].any() and not lab[:, 0].any() and not lab[:, -1].any()
    for m, lab in both("two_combs"):
        assert lab.max() == 2 and np.array_equal(lab != 0, m == 255)
        edge = np.concatenate([m[0], m[-1], m[:, 0], m[:, -1]])
        assert (edge != 255).sum() == 1 and m[0, 31] == 0  # the serpentine's one exit
        assert lab[0, 0] == 1 and lab[2, 2] == 2 and (lab == 2).sum() > 800 and (lab == 1).sum() > 800
    for m, lab in both("lines"):
        assert m.shape == (60, 100) and lab.max() == 30
        assert np.array_equal(lab, np.repeat(np.where(np.arange(60) % 2 == 0, np.arange(60) // 2 + 1, 0), 100).reshape(60, 100))
    for m, lab in both("checker"):
        assert m.shape[0] % 2 == 1 and m.shape[1] % 2 == 1 and lab.max() == 1
        assert (lab[1:-1, 1:-1] == 1).all() and (m[1:-1, 1:-1] == 0).sum() > 500  # every interior hole filled
        ring = np.ones(m.shape, bool)
        ring[1:-1, 1:-1] = False
        assert np.array_equal(lab[ring] != 0, m[ring] == 255)  # border background stays background
    for m, lab in both("diagonals"):
        assert m.shape == (33, 33) and lab.max() == 1 and np.array_equal(lab != 0, m == 255) and (lab != 0).sum() == 65
    for m, lab in both("raster_order"):
        H, W = m.shape
        assert lab.max() == 5 and np.array_equal(lab != 0, m == 255)
        assert lab[0, 50] == 1 and lab[2, 35] == 1 and lab[20, 40] == 1  # the U, first met at its right tip in row 0
        assert lab[1, 0] == 2 and np.nonzero(lab == 2)[1].min() < np.nonzero(lab == 1)[1].min()
        assert lab[4, 40] == 3 and lab[H - 1, 0] == 4 and lab.ravel()[H * W - 1] == 5
    for m, lab in both("border_leak"):
        assert lab.max() == 1 and np.array_equal(lab != 0, m == 255) and m[0, 4] == 0 and lab[4, 4] == 0
        edge_bg = (m[0, :9] == 0).sum() + (m[:9, 0] == 0).sum()
        assert edge_bg == 1 and (m[1:8, 1:8] == 0).all()  # the cavity's only way out is one border pixel
    for m, lab in both("sealed_with_island"):
        assert lab.max() == 1 and m[4, 4] == 255 and (m[1:8, 1:8] == 0).sum() == 48
        assert (lab[:9, :9] == 1).all() and (lab != 0).sum() == 81
    for m, lab in both("near_255"):
        assert set(np.unique(m).tolist()) == {1, 254, 255} and (m == 255).sum() == 5
        assert lab.max() == 5 and np.array_equal(lab != 0, m == 255)
    m, _, _ = CASES["pythagoras@5.0"]
    out, nxt = pure("pythagoras@5.0"), pure("pythagoras_next@5.0+")
    assert (m == 255).sum() == 4 and out.max() == 4 and nxt.max() == 4
    r, c = froc_cases.PYTHAGORAS_SEEDS[0]
    k = out[r, c]
    assert k == nxt[r, c] == 2  # (0, 44) comes first in raster order
    for dr, dc in ((3, 4), (4, 3), (-3, -4), (5, 0), (0, -5), (-5, 0)):  # d2 = 25 is not < 25, and is < 26
        assert out[r + dr, c + dc] == 0 and nxt[r + dr, c + dc] == k, (dr, dc)
    assert out[r + 4, c + 2] == k and nxt[r + 4, c + 2] == k and nxt[r + 5, c + 1] == 0
    assert (out != 0).sum() < (nxt != 0).sum()
    for m, lab in both("root_at_zero"):
        assert m[0, 0] == 255 and lab[0, 0] == 1 and (lab == 1).sum() == 1 and lab.max() == 18 * 19
    for pixel, (r0, c0) in froc_cases.CHUNK_ROOTS.items():
        for m, lab in both(f"roots_on_chunks_{pixel}"):
            assert m.shape == (40, 1025) and lab.max() == (m == 255).sum() == 20 * (513 - c0)
            flat = lab.ravel()
            assert flat[pixel] == (m.ravel()[:pixel] == 255).sum() + 1  # a component of its own, hence a root
            assert (flat[[pixel - 1, pixel + 1]] == 0).all()


def test_structure_of_every_case():
    check_structure()


def test_exact_moments_is_the_per_label_sum():
    for name in ("raster_order@0.5", "open_rings@1.0", "pythagoras@5.0"):
        lab = pure(name)
        want = []
        for k in range(1, int(lab.max()) + 1):
            r, c = (v.astype(np.int64) for v in np.nonzero(lab == k))
            want.append([r.size, r.sum(), c.sum(), (r * r).sum(), (c * c).sum(), (r * c).sum()])
        assert np.array_equal(froc_cases.exact_moments(lab), np.asarray(want, np.int64))
    lab = np.array([[3, -1, 2], [2, 7, 0]], np.int32)  # restricted to 1..2: everything else is ignored
    assert froc_cases.exact_moments(lab, 2).tolist() == [[0] * 6, [2, 1, 2, 1, 4, 0]]


def test_no_itc_decision_at_rounding_distance():
    """computeITCList takes the axes from integer moments, froc_cpu.itc_list from float64 means: the GPU test compares
    the two lists, so no axis of a case may sit on the ITC threshold."""
    for name, (m, res, level) in CASES.items():
        if name.startswith("roots_on_chunks") or name.startswith("root_at_zero"):
            assert pure(name).max() == (m == 255).sum()  # single pixels: every axis is 0
            continue
        thr = 275 / (res * pow(2, level))
        assert all(abs(a - thr) > 1e-6 * thr for a in froc_cpu.major_axes(pure(name))), name


def test_closed_form_lattice_on_a_miniature():
    for H, W in ((64, 66), (65, 64), (7, 9)):
        labels, moments = froc_cases.lattice_expected(H, W)
        m = froc_cases.lattice(H, W)
        for t in (0.5, 1.0):
            assert np.array_equal(froc_cpu.evaluation_mask_pure(m, froc_cases.res_for_threshold(t), froc_cases.LEVEL), labels)
        assert labels.dtype == np.int32 and moments.dtype == np.int64
        assert np.array_equal(moments, froc_cases.exact_moments(labels))
    for H, W in froc_cases.LARGE_LATTICES:  # the two sides of per = (chunks + 1023) / 1024 in the numbering scan
        chunks = (H * W + froc_cases.CHUNK - 1) // froc_cases.CHUNK
        assert (chunks + 1023) // 1024 == (1 if H == 1024 else 2)


def test_pure_matches_live_scipy_on_every_case():
    pytest.importorskip("scipy")
    for name, (m, res, level) in CASES.items():
        assert np.array_equal(pure(name), froc_cpu.evaluation_mask(m, res, level)), name


def test_pure_matches_live_scipy_on_random_masks():
    pytest.importorskip("scipy")
    for m, res, level in froc_cases.random_draws():
        assert np.array_equal(froc_cpu.evaluation_mask_pure(m, res, level), froc_cpu.evaluation_mask(m, res, level)), (m.shape, level)


def test_reference_needs_no_scipy(golden_dir, monkeypatch):
    for mod in [k for k in sys.modules if k == "scipy" or k.startswith("scipy.")]:
        monkeypatch.delitem(sys.modules, mod)
    monkeypatch.setitem(sys.modules, "scipy", None)  # `import scipy` now raises ImportError
    with pytest.raises(ImportError):
        froc_cpu.evaluation_mask(np.zeros((3, 3), np.uint8))
    check_golden_pin(golden_dir)
    pure.cache_clear()
    try:
        check_structure()
    finally:
        pure.cache_clear()
