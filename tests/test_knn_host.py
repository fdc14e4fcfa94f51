"""Host only: the numpy restatement of the k-NN probe (tests/knn_cpu.py) against brute force, the flags of --validate_knn,
and the golden file behind the gates of tests/test_gpu_knn.py."""
import functools
import json
import math
import os

import numpy as np
import pytest

import knn_cases as cases
import knn_cpu as cpu
from ss25_hierarchical_multiscale_image_classification_amd import main as cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_fp32_distances.json")


def brute_topk(row, k):
    """A stable sort with the rule as a comparison function, nothing shared with knn_cpu.topk."""
    def before(a, b):
        sa, sb = row[a], row[b]
        na, nb = math.isnan(sa), math.isnan(sb)
        if na != nb:
            return 1 if na else -1
        if not na and sa != sb:
            return -1 if sa > sb else 1
        return a - b

    return sorted(range(len(row)), key=functools.cmp_to_key(before))[:k]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_topk_of_the_restatement_is_the_ordering_rule(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sim = rng.integers(-3, 4, size=(9, 50)).astype(np.float32)  # few values: many ties
    sim[rng.random(sim.shape) < 0.1] = np.nan
    sim[rng.random(sim.shape) < 0.05] = -np.inf
    sim[rng.random(sim.shape) < 0.05] = np.inf
    sim[0, :] = np.nan
    sim[1, ::2] = -0.0
    sim[1, 1::2] = 0.0
    for k in (1, 7, 50):
        vals, idx = cpu.topk(sim, k)
        for i in range(sim.shape[0]):
            want = brute_topk([float(v) for v in sim[i]], k)
            assert idx[i].tolist() == want, (seed, k, i)
            assert np.array_equal(vals[i], sim[i][want], equal_nan=True)
    assert cpu.topk(sim, 50)[1][1].tolist() == list(range(50))  # -0 == +0: by position


def test_vote_ties_weights_and_temperature_limits():
    lab = np.array([0, 1, 1, 0])
    sim, idx = np.array([[0.5, 0.5]], np.float32), np.array([[0, 1]], np.int32)
    scores, pred = cpu.vote(sim, idx, lab, 0.07, [1.0, 1.0])
    assert scores[0, 0] == scores[0, 1] == 1.0 and pred[0] == 0  # a tie goes to class 0
    scores, pred = cpu.vote(sim, idx, lab, 0.07, [1.0, 1.5])
    assert scores[0].tolist() == [1.0, 1.5] and pred[0] == 1  # the class weights are honoured
    scores, pred = cpu.vote(sim, idx, lab, 0.07, [2.0, 1.5])
    assert pred[0] == 0
    sim = np.array([[1.0, 0.2, -1.0, -1.0]], np.float32)
    idx = np.array([[0, 1, 2, 3]], np.int32)
    for T in (0.01, 10.0):  # the limits of --validate_knn_T: every weight is exp(<= 0)
        scores, pred = cpu.vote(sim, idx, lab, T, [1.0, 1.0])
        assert np.isfinite(scores).all() and (scores >= 0).all() and scores[0, 0] >= 1.0
    s_cold = cpu.vote(sim, idx, lab, 0.01, [1.0, 1.0])[0]
    near = math.exp((float(np.float32(0.2)) - 1.0) * (1.0 / 0.01))
    assert s_cold[0, 0] == 1.0 + math.exp(-200.0) and s_cold[0, 1] == near + math.exp(-200.0)
    scores, pred = cpu.vote(np.array([[np.nan, np.nan]], np.float32), np.array([[0, 3]], np.int32), lab, 0.07, [1.0, 1.0])
    assert np.isnan(scores).all() and pred[0] == 0


def parse(argv):
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    cli.check_validate_knn_args(parser, args)
    return args


@pytest.mark.parametrize("argv", [
    ["--validate_knn", "5"], ["--validate_knn_T", "0.1"], ["--validate_save_knn"],           # without --validate
    ["--validate", "--validate_save_knn"], ["--validate", "--validate_knn_T", "0.1"],         # without --validate_knn
    ["--validate", "--validate_knn", "0"], ["--validate", "--validate_knn", "257"], ["--validate", "--validate_knn", "x"],
    ["--validate", "--validate_knn", "5", "--validate_knn_T", "0.009"], ["--validate", "--validate_knn", "5", "--validate_knn_T", "10.5"],
    ["--validate", "--validate_knn"],
])
def test_the_parser_refuses(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert e.value.code == 2
    assert "validate_knn" in capsys.readouterr().err or "validate_save_knn" in argv[-1]


def test_the_parser_accepts():
    a = parse(["--validate"])
    assert a.validate_knn is None and a.validate_knn_T is None and not a.validate_save_knn
    a = parse(["--validate", "--validate_knn", "1"])
    assert a.validate_knn == 1 and a.validate_knn_T is None
    a = parse(["--validate", "--validate_knn", "256", "--validate_knn_T", "0.01", "--validate_save_knn"])
    assert a.validate_knn == 256 and a.validate_knn_T == 0.01 and a.validate_save_knn
    assert parse(["--validate", "--validate_knn", "20", "--validate_knn_T", "10"]).validate_knn_T == 10.0


def test_main_refuses_with_status_2_before_any_work(capsys):
    for argv in (["--validate_knn", "5"], ["--validate", "--validate_save_knn"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2


def test_the_golden_file_has_every_group_the_gpu_test_reads():
    doc = json.load(open(GOLDEN))
    assert doc["factor"] == 10.0
    for shape in cases.FLOAT64_SHAPES + cases.SPLIT_SHAPES:
        g = doc["per_group"][cases.group_key(shape[0])]
        c = doc["per_case"][cases.shape_id(shape)]
        assert 0 < c["sim"] <= g["sim"] < 1e-6 and 0 < c["inv_norms"] <= g["inv_norms"] < 1e-6
        # a gate below the half ulp of a cosine near 1 would ask more than float32 can give
        assert 10 * g["sim"] > 2.0 ** -24 and 10 * g["inv_norms"] > 2.0 ** -24


def test_the_end_to_end_inputs_are_as_separated_as_the_gpu_test_assumes():
    from ss25_hierarchical_multiscale_image_classification_amd import validate
    x, y = cases.e2e_inputs()
    assert x.shape == (400, 64) and int(y.sum()) == 100
    train, test = validate.stratified_split(y, 42)
    ref = cpu.classify(x, y, train, test, 5, 0.07, validate.balanced_class_weights(y[train]))
    margin = np.abs(ref["scores"][:, 1] - ref["scores"][:, 0]) / (ref["scores"][:, 1] + ref["scores"][:, 0])
    assert margin.min() == 1.0 and np.array_equal(ref["pred"], y[test])
