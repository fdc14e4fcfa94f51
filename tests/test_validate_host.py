"""The host side of --validate (validate.py, main.py) without a GPU: the split rule, the sign rule, the metrics, the command
line's refusals, and the float64 oracle of tests/validate_cpu.py against scikit-learn where it imports."""
import numpy as np
import pytest

import validate_cases as cases
import validate_cpu as cpu
from ss25_hierarchical_multiscale_image_classification_amd import main as cli
from ss25_hierarchical_multiscale_image_classification_amd import validate
from ss25_hierarchical_multiscale_image_classification_amd.mil_train import classification_metrics


def labels_of(n0, n1, seed=0):
    y = np.array([0] * n0 + [1] * n1, np.int64)
    return y[np.random.Generator(np.random.PCG64(seed)).permutation(y.size)]


@pytest.mark.parametrize("n0,n1", [(2, 2), (2, 7), (3, 3), (10, 4), (100, 37), (803, 198)])
def test_split_counts_are_disjoint_sorted_and_seeded(n0, n1):
    y = labels_of(n0, n1)
    train, test = validate.stratified_split(y, 7)
    for cls, n in ((0, n0), (1, n1)):
        assert (y[test] == cls).sum() == max(1, int(np.floor(0.2 * n + 0.5)))
        assert (y[train] == cls).sum() == n - (y[test] == cls).sum() >= 1
    assert not set(train) & set(test) and sorted(set(train) | set(test)) == list(range(n0 + n1))
    assert np.all(np.diff(train) > 0) and (test.size < 2 or np.all(np.diff(test) > 0))
    again = validate.stratified_split(y, 7)
    assert np.array_equal(again[0], train) and np.array_equal(again[1], test)
    if n0 + n1 > 10:
        assert not np.array_equal(validate.stratified_split(y, 8)[1], test)
    ref = cpu.split(y, 7)  # the restated rule
    assert np.array_equal(ref[0], train) and np.array_equal(ref[1], test)


def test_split_is_the_stated_draw():
    y = labels_of(11, 6, seed=3)
    rng = np.random.Generator(np.random.PCG64(5))
    p0 = rng.permutation(np.flatnonzero(y == 0))
    p1 = rng.permutation(np.flatnonzero(y == 1))
    train, test = validate.stratified_split(y, 5)
    assert list(test) == sorted(list(p0[:2]) + list(p1[:1]))  # floor(2.2 + 0.5) = 2, floor(1.2 + 0.5) = 1
    assert list(train) == sorted(list(p0[2:]) + list(p1[1:]))


@pytest.mark.parametrize("y", [[0, 0, 0, 1], [1, 1, 1, 0], [0, 0, 0], [1, 1], [0, 1]])
def test_split_refuses_a_class_of_fewer_than_two_rows(y):
    with pytest.raises(ValueError, match="at least 2"):
        validate.stratified_split(np.array(y), 0)


def test_two_row_classes_give_one_row_each_way():
    train, test = validate.stratified_split(np.array([0, 1, 0, 1]), 1)
    assert train.size == 2 and test.size == 2


def test_sign_rule():
    comp = np.array([[0.1, -0.9, 0.3], [0.5, 0.2, -0.4], [-0.7, 0.7, 0.1], [0.0, 0.0, 0.0]])
    out = validate.flip_signs(comp)
    assert np.array_equal(out[0], -comp[0]) and np.array_equal(out[1], comp[1])
    assert np.array_equal(out[2], -comp[2])  # a tie: the first entry of largest magnitude decides, as numpy's argmax does
    assert np.array_equal(out[3], comp[3])
    assert np.array_equal(out, cpu.flip_signs(comp))
    assert np.array_equal(comp[0], [0.1, -0.9, 0.3])  # the argument is left alone


def test_top_components_of_a_known_covariance():
    rng = np.random.Generator(np.random.PCG64(1))
    q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    cov = q @ np.diag([9.0, 4.0, 1.0, 0.5, 0.3, 0.2]) @ q.T
    ratios, comps = validate.top_components(cov, 2)
    assert np.allclose(ratios, [9 / 15, 4 / 15], rtol=1e-12)
    for k in range(2):
        assert abs(abs(comps[k] @ q[:, k]) - 1) < 1e-12 and comps[k][np.argmax(np.abs(comps[k]))] > 0


def test_metrics_on_a_hand_made_confusion():
    y_true = [1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    y_pred = [1, 1, 1, 0, 0, 0, 0, 0, 1, 1]  # TP 3, FN 1, TN 4, FP 2
    m = classification_metrics(y_true, y_pred)
    assert m["confusion_matrix"] == {"TP": 3, "TN": 4, "FP": 2, "FN": 1}
    assert m["accuracy"] == 0.7 and m["precision"] == 0.6 and m["recall"] == 0.75
    assert abs(m["f1_score"] - 2 * 0.6 * 0.75 / 1.35) < 1e-15
    none = classification_metrics([0, 0], [0, 0])
    assert none["precision"] == none["recall"] == none["f1_score"] == 0.0 and none["accuracy"] == 1.0


def test_balanced_class_weights_are_scikit_learns():
    w = validate.balanced_class_weights([0, 0, 0, 1])
    assert np.array_equal(w, [4 / 6, 4 / 2]) and np.array_equal(w, cpu.balanced_weights([0, 0, 0, 1]))


def test_check_labels():
    assert validate.check_labels(np.array([0, 1, 1], np.uint8)).dtype == np.int64
    for bad in ([0, 1, 2], [-1, 0], [0.0, 1.0], [[0, 1]]):
        with pytest.raises(ValueError):
            validate.check_labels(np.array(bad))


# ---- the command line ----------------------------------------------------------------------------------------------


def test_validate_with_missing_files_prints_the_reference_message(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert cli.main(["--validate"]) == 1
    out = capsys.readouterr().out
    assert "[ERROR] Features or labels not found. Please run feature extraction first." in out
    assert "outside the accelerated hot path" not in out
    np.save("patch_features_2.npy", np.zeros((4, 8), np.float32))  # the labels are still missing
    assert cli.main(["--validate", "--patch_level", "2"]) == 1
    assert cli.main(["--validate", "--patch_level", "all"]) == 1
    assert capsys.readouterr().out.count("Features or labels not found") == 5


def test_validate_is_in_scope_and_the_other_names_are_not(capsys):
    assert "validate" not in cli.OUT_OF_SCOPE
    assert cli.OUT_OF_SCOPE == ("download", "remote", "prepare", "validation", "evaluate", "balance_dataset", "count_tumor_patches",
                                "patch_one_slide", "slide", "move_files", "check_good_downloaded_files")
    for name in cli.OUT_OF_SCOPE:
        argv = [f"--{name}", "x"] if name in ("patch_one_slide", "slide") else [f"--{name}"]
        assert cli.main(argv) == 2
        assert f"--{name} is outside the accelerated hot path" in capsys.readouterr().out
    args = cli.build_parser().parse_args([])
    assert args.validate is False and args.validate_save_pca is False and args.validate_C == 1.0 and args.validate_tol == 1e-4


@pytest.mark.parametrize("labels", [np.array([0, 1, 2, 1]), np.array([0.0, 1.0, 0.0, 1.0]), np.array([-1, 0, 1, 1])])
def test_validate_refuses_labels_other_than_0_and_1(tmp_path, monkeypatch, capsys, labels):
    monkeypatch.chdir(tmp_path)
    np.save("patch_features_3.npy", np.ones((4, 8), np.float32))
    np.save("patch_labels_3.npy", labels)
    assert cli.main(["--validate"]) == 2
    out = capsys.readouterr().out
    assert "[ERROR] --validate, level 3" in out and "0 (normal) and 1 (tumor)" in out
    assert not (tmp_path / "results").exists()


def test_validate_refuses_bad_flag_values_and_shapes(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    np.save("patch_features_3.npy", np.ones((4, 6), np.float32))
    np.save("patch_labels_3.npy", np.array([0, 1, 0, 1]))
    assert cli.main(["--validate", "--validate_C", "0"]) == 2
    assert cli.main(["--validate", "--validate_tol", "-1"]) == 2
    assert cli.main(["--validate"]) == 2  # 6 columns: not a multiple of 4
    assert "feature dimension 6" in capsys.readouterr().out
    np.save("patch_labels_3.npy", np.array([0, 1, 0]))
    assert cli.main(["--validate"]) == 2
    assert "do not agree" in capsys.readouterr().out


# ---- the oracle is scikit-learn's objective ------------------------------------------------------------------------


@pytest.mark.parametrize("n,F,seed", [(1000, 36, 3), cases.E2E[0]])
def test_oracle_agrees_with_scikit_learn(n, F, seed):
    pytest.importorskip("sklearn")
    from sklearn.decomposition import PCA
    from sklearn.linear_model import LogisticRegression

    x, y = cases.make_features(n, F, seed)
    cases.assert_separated(x)
    ref = cpu.run(x, y, cases.SPLIT_SEED, tol=1e-12)
    assert ref["fit"]["converged"] and ref["fit"]["iterations"] <= 12 and ref["accuracy"] < 1.0
    clf = LogisticRegression(class_weight="balanced", tol=1e-10, max_iter=10000).fit(x[ref["train"]].astype(np.float64), y[ref["train"]])
    d = cases.rel(np.concatenate([clf.coef_[0], clf.intercept_]), ref["theta"])
    p = PCA(n_components=2, svd_solver="full").fit(x.astype(np.float64))
    dr, dc = cases.rel(p.explained_variance_ratio_, ref["ratios"]), cases.rel(p.components_, ref["components"])
    print(f"[validate] oracle vs scikit-learn {n}x{F}: optimum {d:.2e}, ratios {dr:.2e}, components {dc:.2e}")
    assert d <= 2e-5  # L-BFGS stopped at its own tolerance: 1e-6 .. 5e-6 measured
    assert dr <= 1e-12 and dc <= 1e-10
    assert np.array_equal(clf.predict(x[ref["test"]].astype(np.float64)), ref["pred"])
