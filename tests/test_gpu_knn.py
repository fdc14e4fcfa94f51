"""The k-NN probe on the device (csrc/knn.hip, include/hipac_knn.h, knn.py, validate.run(knn_k=..)) against the float64
restatement of tests/knn_cpu.py -- never against another native result.

Gates: 10 x the distance numpy's own float32 arithmetic keeps from float64 on exactly these inputs (the rule of
tests/test_gpu_mil_train.py), measured by tests/tools/measure_knn_fp32.py over all pair similarities of the cases of one F and
kept in tests/golden/knn_fp32_distances.json: similarities 1.4e-7 .. 2.4e-7 except F = 2048 (1.8e-8: cosines of 2048-dim
noise are small), inverse norms 1.0e-7 .. 1.6e-7.  Every test prints its figures before it asserts.

Per query of a float64 case: (a) every returned similarity is within the gate of the float64 similarity of the returned
position; (b) the list is sorted by (similarity descending, position ascending) in the device's own numbers and its positions
are distinct; (c) no bank row outside the list has a float64 similarity above that of the list's last entry plus twice the
gate; (d) the inverse norms are within their gate.  No query is excused from any of them.
"""
import json
import os

import numpy as np
import pytest
import torch

import knn_cases as cases
import knn_cpu as cpu
from ss25_hierarchical_multiscale_image_classification_amd import knn, validate
from ss25_hierarchical_multiscale_image_classification_amd import main as cli

pytestmark = pytest.mark.gpu

MEASURED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_fp32_distances.json")))
FACTOR = MEASURED["factor"]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def up(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dtype)


def bits(t):
    return t.view(torch.int32).cpu().numpy()


def search(x, q_rows, b_rows, K, scaled=True):
    """-> (sim, idx, q_scale, b_scale) as numpy arrays, the cosine search of the device."""
    X, Q, B = up(x), up(q_rows), up(b_rows)
    qs, bs = (knn.inv_norms(X, Q), knn.inv_norms(X, B)) if scaled else (None, None)
    sim, idx = knn.topk(X, K, q_rows=Q, b_rows=B, q_scale=qs, b_scale=bs)
    torch.cuda.synchronize()
    return sim.cpu().numpy(), idx.cpu().numpy(), None if qs is None else qs.cpu().numpy(), None if bs is None else bs.cpu().numpy()


def check_against_float64(tag, shape, x, q_rows, b_rows, got):
    F, n_q, n_b, K = shape
    sim, idx, qs, bs = got
    g = MEASURED["per_group"][cases.group_key(F)]
    gate_sim, gate_inv = FACTOR * g["sim"], FACTOR * g["inv_norms"]
    q64, b64 = cpu.inv_norms(x, q_rows), cpu.inv_norms(x, b_rows)
    s64 = cpu.similarities(x, q_rows, b_rows, q64, b64)
    assert sim.shape == idx.shape == (n_q, K) and idx.min() >= 0 and idx.max() < n_b
    err_sim = np.abs(sim.astype(np.float64) - np.take_along_axis(s64, idx.astype(np.int64), axis=1)).max()  # (a)
    err_inv = max(np.abs(qs / q64 - 1).max(), np.abs(bs / b64 - 1).max())  # (d)
    sorted_ok = all((sim[i, t] > sim[i, t + 1]) or (sim[i, t] == sim[i, t + 1] and idx[i, t] < idx[i, t + 1])
                    for i in range(n_q) for t in range(K - 1))  # (b)
    distinct = all(len(set(idx[i].tolist())) == K for i in range(n_q))
    outside = np.array(s64, copy=True)
    np.put_along_axis(outside, idx.astype(np.int64), -np.inf, axis=1)
    last64 = np.take_along_axis(s64, idx[:, -1:].astype(np.int64), axis=1)[:, 0]
    excess = (outside.max(axis=1) - last64).max() if n_b > K else -np.inf  # (c)
    same_lists = float(np.mean([np.array_equal(idx[i], cpu.topk(s64[i:i + 1], K)[1][0]) for i in range(n_q)]))
    print(f"[knn] {tag}: similarity error {err_sim:.2e} / {gate_sim:.2e}, inverse norms {err_inv:.2e} / {gate_inv:.2e}, "
          f"best row left out exceeds the last one kept by {excess:.2e} / {2 * gate_sim:.2e}, sorted {sorted_ok}, distinct {distinct}, "
          f"lists equal to float64's {same_lists:.3f}")
    assert err_sim <= gate_sim and err_inv <= gate_inv
    assert sorted_ok and distinct
    assert excess <= 2 * gate_sim


def test_exact_ties_go_to_the_lower_position():
    x, q_rows, b_rows = cases.tie_inputs()
    assert len(q_rows) == 33 and len(b_rows) == 300
    s64 = cpu.similarities(x, q_rows, b_rows)  # integers: exact in float32 too
    assert np.array_equal(s64, s64.astype(np.float32).astype(np.float64))
    for K in (1, 5, 64):
        sim, idx, _, _ = search(x, q_rows, b_rows, K, scaled=False)
        want_sim, want_idx = cpu.topk(s64, K)
        ties = int((want_sim[:, :-1] == want_sim[:, 1:]).sum()) if K > 1 else 0
        print(f"[knn] ties, K = {K}: positions differing {int((idx != want_idx).sum())}, similarities differing "
              f"{int((sim != want_sim).sum())}, adjacent equal similarities in the lists {ties}")
        assert np.array_equal(idx, want_idx) and np.array_equal(sim.astype(np.float64), want_sim)


@pytest.mark.parametrize("shape", cases.FLOAT64_SHAPES, ids=[cases.shape_id(s) for s in cases.FLOAT64_SHAPES])
def test_lists_match_float64(shape):
    x, q_rows, b_rows = cases.float64_inputs(*shape)
    check_against_float64(cases.shape_id(shape), shape, x, q_rows, b_rows, search(x, q_rows, b_rows, shape[3]))


@pytest.mark.parametrize("shape", cases.SPLIT_SHAPES, ids=[cases.shape_id(s) for s in cases.SPLIT_SHAPES])
def test_split_and_merge(shape):
    F, n_q, n_b, K = shape
    lib = knn.load_knn_library()
    splits = lib.hipac_knn_bank_splits(n_q, n_b, F, K)
    per_group = -(-n_b // splits)
    print(f"[knn] {cases.shape_id(shape)}: {splits} column groups of about {per_group} rows")
    assert splits >= 2
    if K == 250:
        assert K < per_group <= K + 6  # just above K in every group
    x, q_rows, b_rows = cases.float64_inputs(*shape)
    got = search(x, q_rows, b_rows, K)
    check_against_float64(cases.shape_id(shape), shape, x, q_rows, b_rows, got)
    # the same queries among enough others that the bank is not cut: the same bits
    qt = 128 if K <= 64 else 32
    n_pad = 512 * qt
    assert lib.hipac_knn_bank_splits(n_pad, n_b, F, K) == 1
    padded = np.concatenate([q_rows, np.resize(b_rows, n_pad - n_q)]).astype(np.int32)
    sim1, idx1, _, _ = search(x, padded, b_rows, K)
    assert np.array_equal(sim1[:n_q].view(np.int32), got[0].view(np.int32)) and np.array_equal(idx1[:n_q], got[1])


def test_similarity_bits_do_not_depend_on_position():
    F = 72
    rng = np.random.Generator(np.random.PCG64(7))
    x = (0.7 * rng.standard_normal((21000, F))).astype(np.float32)
    a, b = 17, 18
    x[b] = 3 * x[a]  # the pair is every list's first entry, whatever else is in the bank
    others = np.arange(100, 21000, dtype=np.int32)
    seen = {}

    def run(tag, q_rows, q_at, b_rows, b_at, K):
        sim, idx, _, _ = search(x, np.asarray(q_rows, np.int32), np.asarray(b_rows, np.int32), K)
        assert idx[q_at, 0] == b_at, tag
        seen[tag] = int(sim[q_at, :1].view(np.int32)[0])

    run("alone", [a], 0, [b], 0, 1)
    for at in (0, 31, 32, 127):
        q = others[:128].copy()
        q[at] = a
        run(f"query at {at}", q, at, np.concatenate([others[200:263], [b]]), 63, 5)
    for n_b in (64, 65, 1000):
        bank = others[300:300 + n_b].copy()
        bank[n_b // 2] = b
        for K in (1, min(n_b, 256)):
            run(f"n_b {n_b}, K {K}", [others[5], a], 1, bank, n_b // 2, K)
    bank = others[:20000].copy()
    bank[12345] = b
    assert knn.load_knn_library().hipac_knn_bank_splits(5, 20000, F, 20) >= 2
    run("split", [others[1], others[2], a, others[3], others[4]], 2, bank, 12345, 20)
    print("[knn] bits of the pair's similarity:", {k: hex(v & 0xffffffff) for k, v in seen.items()})
    assert len(set(seen.values())) == 1, seen


def test_nan_and_zero_rows():
    rng = np.random.Generator(np.random.PCG64(11))
    x = (0.7 * rng.standard_normal((50, 16))).astype(np.float32)
    x[7, 3] = np.nan  # bank position 7
    x[45] = 0.0       # query 1: a zero row
    x[46, 0] = np.nan  # query 2: a NaN row
    x[9] = 0.0        # bank position 9: a zero row
    b_rows, q_rows = np.arange(40, dtype=np.int32), np.array([44, 45, 46], np.int32)
    sim40, idx40, qs, bs = search(x, q_rows, b_rows, 40)
    sim39, idx39, _, _ = search(x, q_rows, b_rows, 39)
    print(f"[knn] NaN bank row: last of 40 at position {idx40[0, -1]} (similarity {sim40[0, -1]}), in the 39: {bool((idx39[0] == 7).any())}; "
          f"zero query: similarities {np.unique(sim40[1, :39])}; inverse norm of a zero row {qs[1]:.3g}")
    assert idx40[0, -1] == 7 and np.isnan(sim40[0, -1]) and not np.isnan(sim40[0, :-1]).any()
    assert not (idx39[0] == 7).any() and np.array_equal(idx39[0], idx40[0, :39])
    big = np.float32(1) / np.float32(1e-12)
    assert qs[1] == big and bs[9] == big
    assert (sim40[1, :39] == 0).all() and idx40[1].tolist() == [p for p in range(40) if p != 7] + [7]  # 0 everywhere: by position
    assert (sim40[0][idx40[0] == 9] == 0).all()
    assert np.isnan(sim40[2]).all() and idx40[2].tolist() == list(range(40))  # NaN everywhere: by position
    labels = up((np.arange(40) % 2).astype(np.int32))
    scores, pred = knn.vote(up(sim40), up(idx40), labels, 0.07, [1.0, 1.0])
    torch.cuda.synchronize()
    scores, pred = scores.cpu().numpy(), pred.cpu().numpy()
    assert np.isnan(scores[2]).all() and pred[2] == 0  # a NaN query row
    want, want_pred = cpu.vote(sim40[1:2, :39], idx40[1:2, :39], np.arange(40) % 2, 0.07, [1.0, 1.0])
    got, got_pred = knn.vote(up(sim40[1:2, :39]), up(idx40[1:2, :39]), labels, 0.07, [1.0, 1.0])
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_pred.cpu().numpy(), want_pred)


def test_vote_matches_float64_and_a_tie_goes_to_class_0():
    shape = (512, 65, 1000, 20)
    x, q_rows, b_rows = cases.float64_inputs(*shape)
    sim, idx, _, _ = search(x, q_rows, b_rows, shape[3])
    rng = np.random.Generator(np.random.PCG64(5))
    labels = (rng.random(1000) < 0.3).astype(np.int32)
    worst = 0.0
    for T, cw in ((0.07, [0.7, 1.9]), (0.01, [1.0, 1.0]), (10.0, [2.0, 0.6])):
        scores, pred = knn.vote(up(sim), up(idx), up(labels), T, cw)
        torch.cuda.synchronize()
        want, want_pred = cpu.vote(sim, idx, labels, T, cw)
        scores = scores.cpu().numpy()
        nz = want != 0
        assert np.array_equal(scores == 0, ~nz)
        worst = max(worst, float(np.abs(scores[nz] / want[nz] - 1).max()))
        print(f"[knn] vote T = {T}: relative error of the scores {worst:.2e} / 1e-12, predictions differing "
              f"{int((pred.cpu().numpy() != want_pred).sum())}, positives {int(want_pred.sum())} of {want_pred.size}")
        assert worst <= 1e-12 and np.array_equal(pred.cpu().numpy(), want_pred)
    tie_sim, tie_idx = np.array([[0.5, 0.5], [0.5, 0.25]], np.float32), np.array([[0, 1], [1, 0]], np.int32)
    scores, pred = knn.vote(up(tie_sim), up(tie_idx), up(np.array([0, 1], np.int32)), 0.07, [1.0, 1.0])
    scores, pred = scores.cpu().numpy(), pred.cpu().numpy()
    assert scores[0, 0] == scores[0, 1] == 1.0 and pred.tolist() == [0, 1]


def test_twice_the_same():
    shape = (512, 257, 5000, 64)
    x, q_rows, b_rows = cases.float64_inputs(*shape)
    X, Q, B = up(x), up(q_rows), up(b_rows)
    labels = up((np.arange(5000) % 3 == 0).astype(np.int32))
    outs = []
    for _ in range(2):
        qs, bs = knn.inv_norms(X, Q), knn.inv_norms(X, B)
        sim, idx = knn.topk(X, 64, q_rows=Q, b_rows=B, q_scale=qs, b_scale=bs)
        scores, pred = knn.vote(sim, idx, labels, 0.07, [0.75, 1.5])
        torch.cuda.synchronize()
        outs.append((bits(qs), bits(bs), bits(sim), idx.cpu().numpy(), scores.view(torch.int64).cpu().numpy(), pred.cpu().numpy()))
    assert all(np.array_equal(u, v) for u, v in zip(*outs))


_e2e = {}


def e2e():
    """The end-to-end inputs with one test row made a copy of a training row, and the float64 restatement; computed once."""
    if not _e2e:
        x, y = cases.e2e_inputs()
        train, test = validate.stratified_split(y, 42)
        twin = int(train[y[train] == y[test[0]]][3])
        x[test[0]] = x[twin]
        class_w = validate.balanced_class_weights(y[train])
        _e2e.update(x=x, y=y, train=train, test=test, twin=twin, ref=cpu.classify(x, y, train, test, 5, 0.07, class_w))
    return _e2e


def test_run_matches_the_float64_restatement():
    c = e2e()
    ref, y, test = c["ref"], c["y"], c["test"]
    margin = np.abs(ref["scores"][:, 1] - ref["scores"][:, 0]) / (ref["scores"][:, 1] + ref["scores"][:, 0])
    print(f"[knn] end to end: smallest vote margin of the restatement {margin.min():.3f}, accuracy {np.mean(ref['pred'] == y[test]):.4f}")
    assert margin.min() >= 0.05
    res = validate.run(c["x"], y, seed=42, knn_k=5)
    kn = res["knn"]
    want = validate.classification_metrics(y[test], ref["pred"].astype(np.int64))
    assert kn["k"] == 5 and kn["temperature"] == 0.07 and kn["n_train"] == c["train"].size and kn["n_test"] == test.size
    for key in ("accuracy", "precision", "recall", "f1_score", "confusion_matrix"):
        assert kn[key] == want[key], key
    assert kn["accuracy"] == 1.0
    table = kn["neighbours"]
    assert table.dtype == np.int32 and table.shape == (test.size, 6) and np.array_equal(table[:, 0], test)
    assert np.isin(table[:, 1:], c["train"]).all() and table[0, 1] == c["twin"]
    assert "knn" not in validate.run(c["x"], y, seed=42) and "knn_skipped" not in validate.run(c["x"], y, seed=42)
    few = validate.run(c["x"][:12], np.array([0] * 9 + [1] * 3), seed=42, knn_k=20)
    assert "knn" not in few and "20" in few["knn_skipped"]
    one = validate.run(c["x"][:12], np.array([0] * 11 + [1]), seed=42, knn_k=5)
    assert "knn" not in one and one["knn_skipped"] == one["probe_skipped"]


def test_cli_writes_the_knn_report_and_only_when_asked(tmp_path, monkeypatch, capsys):
    c = e2e()
    monkeypatch.chdir(tmp_path)
    np.save("patch_features_3.npy", c["x"])
    np.save("patch_labels_3.npy", c["y"])
    assert cli.main(["--validate", "--patch_level", "3", "--validate_knn", "5", "--validate_save_knn"]) == 0
    text = capsys.readouterr().out
    assert "[INFO] k-NN (k = 5, T = 0.07) accuracy: 1.0000" in text
    assert text.index("[INFO] Logistic Regression Accuracy:") < text.index("[INFO] k-NN (k = 5")
    doc = json.load(open(os.path.join("results", "validate_3.json")))
    assert sorted(doc["knn"]) == ["accuracy", "confusion_matrix", "f1_score", "k", "n_test", "n_train", "precision", "recall", "temperature"]
    assert doc["knn"]["k"] == 5 and doc["knn"]["n_train"] + doc["knn"]["n_test"] == 400
    table = np.load(os.path.join("results", "knn_3.npy"))
    assert table.dtype == np.int32 and table.shape == (c["test"].size, 6)
    assert table[0, 0] == c["test"][0] and table[0, 1] == c["twin"]  # the first neighbour of a duplicated row is its duplicate
    os.remove(os.path.join("results", "knn_3.npy"))

    assert cli.main(["--validate", "--patch_level", "3"]) == 0
    text = capsys.readouterr().out
    assert "knn" not in json.load(open(os.path.join("results", "validate_3.json"))) and not os.path.exists(os.path.join("results", "knn_3.npy"))
    res = validate.run(c["x"], c["y"], seed=42, knn_k=5)
    del res["knn"]
    plain = validate.report(res)
    want = capsys.readouterr().out
    assert "k-NN" not in text and text.endswith(want) and "knn" not in plain
    assert text[:len(text) - len(want)].count("\n") == 3  # the three lines cmd_validate prints itself
