"""The bootstrap of ``--run_evaluation`` on the device (csrc/eval_ci.hip via froc_ci.py) against the numpy restatement in
tests/eval_ci_cpu.py: the draws, every replicate's integers (exactly: there is no tolerance anywhere), determinism,
independence of B and of where a call starts, the argument errors, and ``--eval_roc --eval_bootstrap`` end to end."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import eval_ci_cpu as ref
from ss25_hierarchical_multiscale_image_classification_amd import capi, froc_ci

pytestmark = pytest.mark.gpu

B = 64
NAMES = sorted(ref.all_tables())


@functools.lru_cache(maxsize=None)
def expected(name):
    t = ref.all_tables()[name]
    return ref.integers_all(t, ref.draws(ref.SEED, 0, B, len(t["names"])))


def package_tables(name):
    t = ref.all_tables()[name]
    return froc_ci.build_tables(ref.froc_data(t), t["scores"], t["labels"])


def same(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("S", [1, 2, 7, 129, 300, 4096])
def test_counts_equal_the_numpy_draws(S):
    for n, first in ((1, 0), (5, 0), (5, 1 << 20)):
        got = froc_ci.draw_counts(ref.SEED, first, n, S)
        assert got.dtype == np.int32 and got.shape == (n, S)
        assert (got.sum(1) == S).all() and (got >= 0).all()
        assert np.array_equal(got, ref.draws(ref.SEED, first, n, S)), (S, n, first)
    if S >= 129:  # either key word changes the draws
        for other in (ref.SEED + 1, ref.SEED ^ (1 << 40)):
            assert not np.array_equal(froc_ci.draw_counts(ref.SEED, 0, 1, S), froc_ci.draw_counts(other, 0, 1, S))


@pytest.mark.parametrize("name", NAMES)
def test_bootstrap_integers_equal_the_restatement_exactly(name):
    got = froc_ci.bootstrap_integers(package_tables(name), ref.SEED, 0, B)
    want = expected(name)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k, np.flatnonzero((got[k] != want[k]).reshape(B, -1).any(1)))
    assert (got["n_pos"] + got["n_neg"] == len(ref.all_tables()[name]["names"])).all()


@pytest.mark.parametrize("name", ["e_129_cases", "f_70000_events_300_cases"])
def test_two_runs_are_identical(name):
    pk = package_tables(name)
    assert same(froc_ci.bootstrap_integers(pk, ref.SEED, 0, B), froc_ci.bootstrap_integers(pk, ref.SEED, 0, B))


def test_a_replicate_depends_neither_on_B_nor_on_the_start():
    pk = package_tables("e_129_cases")
    eight, one = froc_ci.bootstrap_integers(pk, ref.SEED, 0, 8), froc_ci.bootstrap_integers(pk, ref.SEED, 5, 1)
    assert same({k: v[5:6] for k, v in eight.items()}, one)
    assert same({k: v[:8] for k, v in expected("e_129_cases").items()}, eight)
    other = froc_ci.bootstrap_integers(pk, ref.SEED ^ 1, 5, 1)  # and on the seed it does
    assert not np.array_equal(other["tp_at_rate"], one["tp_at_rate"]) or not np.array_equal(other["u2"], one["u2"])


def test_fewer_rates_and_other_rates():
    t, pk = ref.all_tables()["e_129_cases"], package_tables("e_129_cases")
    rates = (3, 32, 1)
    got = froc_ci.bootstrap_integers(pk, ref.SEED, 0, 4, rates4=rates)
    assert same(got, ref.integers_all(t, ref.draws(ref.SEED, 0, 4, 129), rates))


def test_bad_arguments_raise():
    lib = froc_ci.load_eval_ci_library()
    pk = package_tables("b_one_tumour_one_hit")
    for n in (0, 65537):
        with pytest.raises(capi.HipacError):
            froc_ci.bootstrap_integers(pk, 1, 0, n)
        with pytest.raises(capi.HipacError):
            froc_ci.draw_counts(1, 0, n, 7)
    buf = torch.zeros(4097 * 2, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert lib.hipac_eval_ci_counts(1, 0, 0, 7, buf.data_ptr(), None) == -1
    assert lib.hipac_eval_ci_counts(1, 0, 65537, 7, buf.data_ptr(), None) == -1
    assert lib.hipac_eval_ci_counts(1, 0, 1, 4097, buf.data_ptr(), None) == -1
    with pytest.raises(capi.HipacError):
        froc_ci.draw_counts(1, 0, 1, 4097)
    rates = (C.c_int32 * 6)(*froc_ci.RATES4)

    def call(ev=buf.data_ptr(), tum=buf.data_ptr(), S=7, n=3, nb=1):
        return lib.hipac_eval_ci_bootstrap(ev, buf.data_ptr(), buf.data_ptr(), n, tum, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), S, 1, 0, nb,
                                           C.cast(rates, C.c_void_p), 6, out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                           out.data_ptr(), None)

    assert call(nb=0) == -1 and call(nb=65537) == -1 and call(S=4097) == -1
    assert call(ev=None) == -1 and b"null" in lib.hipac_last_error()
    assert call(tum=None) == -1 and b"null" in lib.hipac_last_error()
    with pytest.raises(capi.HipacError):
        froc_ci.build_tables((["x"] * 4097, [[]] * 4097, [[]] * 4097, [0] * 4097), [0.0] * 4097, [0] * 4097)
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------

M5 = 96  # side of the level-5 mask; level 0 is 32 times that


def tumour_mask(bars, dots):
    m = np.zeros((M5, M5), np.uint8)
    for r, c, h, w in bars:  # lesions: long enough to count as tumours
        m[r:r + h, c:c + w] = 255
    for r, c in dots:  # isolated tumour cells: 3 x 3 pixels
        m[r:r + 3, c:c + 3] = 255
    return m


def at(r, c):
    """level-0 (x, y) of the centre of level-5 pixel (r, c)"""
    return c * 32 + 16, r * 32 + 16


def write_root(tmp_path):
    from ss25_hierarchical_multiscale_image_classification_amd import tiff_pyramid

    root = tmp_path / "data"
    os.makedirs(root / "test" / "mask")
    csvs = tmp_path / "models" / "first_model" / "model_predictions_csv"
    os.makedirs(csvs)
    tumours = {
        "tumor_001": (tumour_mask([(20, 10, 8, 50)], [(70, 70)]), [(0.9, at(24, 30)), (0.7, at(23, 40)), (0.6, at(71, 71)), (0.7, at(60, 10)), (0.2, at(5, 5))]),
        "tumor_002": (tumour_mask([(10, 20, 50, 8), (70, 10, 8, 60)], []), [(0.7, at(30, 24)), (0.5, at(90, 90)), (0.1, at(2, 80))]),
        "test_003": (tumour_mask([(40, 30, 10, 45)], [(5, 5), (80, 80)]), [(0.3, at(6, 6)), (0.4, at(50, 90)), (0.4, at(20, 20)), (0.3, at(45, 50))]),
    }
    for case, (m5, dets) in tumours.items():
        levels = [np.repeat(np.repeat(m5, 1 << (5 - k), 0), 1 << (5 - k), 1) for k in range(6)]
        tiff_pyramid.write_tiled_tiff(str(root / "test" / "mask" / f"{case}_Mask.tif"), levels, compression="deflate")
        with open(csvs / f"{case}.csv", "w") as f:
            for p, (x, y) in dets:
                f.write(f"{p},{x},{y}\n")
    normals = {"normal_001": [0.8, 0.1], "normal_002": [], "normal_003": [0.7, 0.3, 0.3, 0.2], "test_004": [0.4]}
    for case, probs in normals.items():
        with open(csvs / f"{case}.csv", "w") as f:
            for i, p in enumerate(probs):
                f.write(f"{p},{100 + 500 * i},{200 + 300 * i}\n")
    return root, {**{k: [p for p, _ in v[1]] for k, v in tumours.items()}, **normals}, set(tumours)


def test_run_evaluation_with_roc_and_bootstrap_end_to_end(tmp_path, monkeypatch, capsys):
    from ss25_hierarchical_multiscale_image_classification_amd import main

    root, probs, tumours = write_root(tmp_path)
    monkeypatch.chdir(tmp_path)
    assert main.main(["--run_evaluation", "--data_root", str(root)]) == 0
    plain = open(tmp_path / "froc_results.json", "rb").read()
    assert not os.path.exists(tmp_path / "roc_results.json") and not os.path.exists(tmp_path / "bootstrap_results.json")
    plain_out = capsys.readouterr().out
    NB, SEED, CI = 200, 3, 95.0
    assert main.main(["--run_evaluation", "--data_root", str(root), "--eval_roc", "--eval_bootstrap", str(NB), "--seed", str(SEED)]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain_out) and len(out.splitlines()) == len(plain_out.splitlines()) + 2 + 1 + 6 + 1 + 1
    assert open(tmp_path / "froc_results.json", "rb").read() == plain
    res = json.loads(plain)
    roc, boot = json.load(open(tmp_path / "roc_results.json")), json.load(open(tmp_path / "bootstrap_results.json"))

    # the restatement, from the cases as froc_results.json lists them
    cases = [c["case"][:-4] for c in res["cases"]]
    assert cases == sorted(probs) and len(cases) == 7
    t = {"names": [c["case"] for c in res["cases"]], "fps": [c["FP_probs"] for c in res["cases"]],
         "tps": [np.asarray(c["TP_probs"], np.float32) for c in res["cases"]], "ntum": [c["num_of_tumors"] for c in res["cases"]],
         "labels": [int(c in tumours) for c in cases], "scores": [max(probs[c]) if probs[c] else 0.0 for c in cases]}
    assert sum(t["ntum"]) == 4 and sum(len(a) for a in t["tps"]) == 7  # four lesions, three isolated tumour cells
    assert sum(float(v) > 0 for a in t["tps"] for v in a) == 3  # three lesions are hit; the hit on an ITC counts nowhere
    assert roc["cases"] == [{"case": c, "label": y, "score": s} for c, y, s in zip(cases, t["labels"], t["scores"])]
    six, score, auc = ref.composition(t, np.ones(7, np.int64))
    thr = sorted(set(t["scores"]), reverse=True)
    y, s = np.asarray(t["labels"]), np.asarray(t["scores"])
    assert roc["thresholds"] == [None] + thr and (roc["n_pos"], roc["n_neg"]) == (3, 4)
    assert roc["tpr"] == [0.0] + [int((s[y == 1] >= v).sum()) / 3.0 for v in thr]
    assert roc["fpr"] == [0.0] + [int((s[y == 0] >= v).sum()) / 4.0 for v in thr]
    assert roc["auc"] == auc and 0.0 < auc < 1.0
    assert score == res["froc_score"]

    fin = froc_ci.finish(ref.integers_all(t, ref.draws(SEED, 0, NB, 7)))

    def entry(value, reps):
        ok = reps[~np.isnan(reps)]
        lo, hi = np.percentile(ok, [50.0 - CI / 2.0, 50.0 + CI / 2.0])
        return {"value": value, "lo": float(lo), "hi": float(hi), "undefined": int(np.isnan(reps).sum())}

    assert (boot["replicates"], boot["seed"], boot["ci"]) == (NB, SEED, CI)
    assert boot["froc_score"] == entry(score, fin["froc_score"])
    assert boot["sensitivity_at"] == [entry(six[i], fin["sensitivity_at"][:, i]) for i in range(6)]
    assert boot["auc"] == entry(auc, fin["auc"])
    drawn = ref.draws(SEED, 0, NB, 7)
    no_tumour, no_normal = int((drawn[:, y == 1].sum(1) == 0).sum()), int((drawn[:, y == 0].sum(1) == 0).sum())
    assert boot["froc_score"]["undefined"] == no_tumour > 0 and boot["auc"]["undefined"] == no_tumour + no_normal
    assert boot["froc_score"]["lo"] <= score <= boot["froc_score"]["hi"]
    for r in range(0, NB, 25):  # and the restatement is the composition, here too
        c6, cs, ca = ref.composition(t, ref.draws(SEED, r, 1, 7)[0])
        assert np.array_equal(fin["sensitivity_at"][r], c6, equal_nan=True) and np.array_equal(fin["froc_score"][r], cs, equal_nan=True)
        assert np.array_equal(fin["auc"][r], ca, equal_nan=True)
