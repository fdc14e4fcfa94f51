"""Host side of the MIL training loop (mil_train.py): the split, the rows / offsets of an epoch, the metrics, the parser.
Nothing here touches a GPU."""
import numpy as np
import pytest

from ss25_hierarchical_multiscale_image_classification_amd import main as cli
from ss25_hierarchical_multiscale_image_classification_amd import mil_train


@pytest.mark.parametrize("n", [1, 2, 9, 10, 11, 57, 60, 1000])
def test_split_sizes_disjoint_seeded(n):
    tr, va, te = mil_train.split_bags(n, seed=3)
    assert len(va) == len(te) == int(0.1 * n)
    assert len(tr) == n - len(va) - len(te) >= 1
    assert sorted(np.concatenate([tr, va, te]).tolist()) == list(range(n))  # disjoint and complete
    again = mil_train.split_bags(n, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip((tr, va, te), again))
    if n >= 57:
        assert not np.array_equal(tr, mil_train.split_bags(n, seed=4)[0])


def test_split_refuses_no_bags():
    with pytest.raises(ValueError):
        mil_train.split_bags(0)


def bags_fixture():
    sizes = [1, 5, 100, 101, 250, 37, 12, 400, 3, 64]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    order = np.random.default_rng(0).permutation(int(offsets[-1])).astype(np.int64)  # bag rows are scattered in the matrix
    return sizes, offsets, order


@pytest.mark.parametrize("bag_size", [None, 1, 100, 1000])
def test_epoch_rows_and_offsets(bag_size):
    sizes, offsets, order = bags_fixture()
    train = [0, 2, 3, 4, 5, 7, 9]
    steps = list(mil_train.epoch_batches(train, order, offsets, epoch=2, seed=5, bags_per_step=3, bag_size=bag_size))
    assert [len(g) for _, _, g in steps] == [3, 3, 1]
    assert sorted(int(b) for _, _, g in steps for b in g) == train  # every training bag once per epoch
    for rows, offs, group in steps:
        assert rows.dtype == np.int32 and offs[0] == 0 and offs[-1] == len(rows) and len(offs) == len(group) + 1
        for k, b in enumerate(group):
            r = rows[offs[k]:offs[k + 1]]
            members = order[offsets[b]:offsets[b + 1]]
            assert len(r) == (sizes[b] if bag_size is None else min(sizes[b], bag_size)) >= 1
            assert len(set(r.tolist())) == len(r)  # no repeats
            assert set(r.tolist()) <= set(members.tolist())  # a subset of that bag
    again = list(mil_train.epoch_batches(train, order, offsets, epoch=2, seed=5, bags_per_step=3, bag_size=bag_size))
    for (r0, o0, g0), (r1, o1, g1) in zip(steps, again):
        assert np.array_equal(r0, r1) and np.array_equal(o0, o1) and np.array_equal(g0, g1)
    other = list(mil_train.epoch_batches(train, order, offsets, epoch=3, seed=5, bags_per_step=3, bag_size=bag_size))
    assert any(not np.array_equal(a[2], b[2]) for a, b in zip(steps, other))  # another epoch, another shuffle


def test_metrics_follow_the_reference_definitions():
    t = np.array([1, 1, 1, 0, 0, 0, 0, 1])
    p = np.array([1, 0, 1, 0, 1, 0, 0, 1])
    m = mil_train.classification_metrics(t, p)
    assert m["confusion_matrix"] == {"TP": 3, "TN": 3, "FP": 1, "FN": 1}
    assert m["accuracy"] == 6 / 8 and m["precision"] == 3 / 4 and m["recall"] == 3 / 4
    assert m["f1_score"] == pytest.approx(2 * 0.75 * 0.75 / 1.5)
    for v in (m["accuracy"], m["precision"], m["recall"], m["f1_score"]):
        assert type(v) is float
    assert all(type(v) is int for v in m["confusion_matrix"].values())


def test_metrics_zero_denominators():
    m = mil_train.classification_metrics([0, 0, 1], [0, 0, 0])  # nothing predicted positive
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["f1_score"] == 0.0 and m["accuracy"] == 2 / 3
    m = mil_train.classification_metrics([0, 0, 0], [0, 1, 0])  # no positive exists
    assert m["recall"] == 0.0 and m["precision"] == 0.0 and m["f1_score"] == 0.0
    m = mil_train.classification_metrics([0, 0], [0, 0])
    assert m["accuracy"] == 1.0 and m["f1_score"] == 0.0 and m["confusion_matrix"] == {"TP": 0, "TN": 2, "FP": 0, "FN": 0}


def test_parser_accepts_the_mil_flags():
    a = cli.build_parser().parse_args(["--train_mil", "--mil_pooling", "max", "--patch_level", "2"])
    assert a.train_mil and not a.predict_mil and a.mil_pooling == "max" and a.patch_level == "2"
    assert a.mil_epochs == 50 and a.mil_bags_per_step == 32 and a.mil_bag_size is None and not a.mil_by_slide
    a = cli.build_parser().parse_args(["--predict_mil", "--mil_model", "m.pth", "--mil_bag_size", "100", "--mil_by_slide"])
    assert a.predict_mil and a.mil_model == "m.pth" and a.mil_bag_size == 100 and a.mil_by_slide
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--train_mil", "--mil_pooling", "median"])


@pytest.mark.parametrize("flag", ["--train_mil", "--predict_mil"])
def test_patch_level_all_is_refused_without_a_gpu(flag, capsys):
    assert cli.main([flag, "--patch_level", "all"]) != 0
    assert "one level" in capsys.readouterr().out


def test_missing_triple_is_reported(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert cli.main(["--train_mil", "--patch_level", "2"]) != 0
    assert "patch_features_2.npy" in capsys.readouterr().out
