"""The native MIL training step (csrc/mil_train.hip, mil_train.NativeMILTrainer) against torch autograd in float64 on the
CPU over ``mil.MILClassifier`` in ``train()`` mode, one bag per forward (tests/mil_train_cases.py) -- never against
the native forward.

Tolerances.  The fp32 step differs from the float64 yardstick by summation order only, so each tensor is gated at
10 x the distance torch's OWN float32 autograd keeps from its float64 autograd on exactly these inputs, metric
max|a - b| / max|b|; the factor is the one tests/test_gpu_train.py leaves between its measured 5e-5 and its 5e-4 gate.
The distances are measured on the CPU by tests/tools/measure_mil_train_fp32.py and kept in
tests/golden/mil_train_fp32_distances.json.  A gate is formed over the cases that run the SAME computation -- same
(F, A, hidden, C), same pooling; they differ in class weights, row index and the two-batch accumulate case -- and takes
the largest of their figures: one case's figure is one draw of rounding noise (torch's float32 lands 6.0e-9 from float64 on
classifier.2.bias in attention-nw-perm, a tenth of float32's half-ulp, which no float32 computation can be held to).
Nothing is pooled across poolings or dims.  Measured fp32-vs-fp64 -> gate (x 10), attention pooling:

    (512,128,128,2):  attn_V.weight 3.0e-7   attn_V.bias 5.7e-7   attn_U.weight 3.3e-7   classifier.0.weight 1.8e-7
                      .0.bias 1.4e-7   .2.weight 2.4e-7   .2.bias 6.2e-7   logits 2.6e-7
    (128,64,32,3):    attn_V.weight 3.6e-7   attn_V.bias 4.1e-7   attn_U.weight 6.1e-7   classifier.* 6.6e-8 .. 1.3e-7   logits 1.3e-7
    (1024,256,256,2): attn_V.weight 3.0e-7   attn_V.bias 5.2e-7   attn_U.weight 3.9e-7   classifier.* 1.1e-7 .. 3.4e-7   logits 2.4e-7
    mean / max: classifier.* and logits 3.5e-8 .. 4.3e-7 (see the json)

aggregator.attn_U.bias has gradient 0 in exact arithmetic (a constant added to every score of a bag cancels in the
softmax); float64 autograd leaves ~1e-18 there and float32 ~1e-9, so it is gated absolutely at 10 x what float32
autograd leaves on the same inputs: 1.3e-9 -> 1.3e-8 at the reference dims, 2.0e-10 -> 2.0e-9 and 5.3e-10 -> 5.3e-9 at the
other two.  Loss: 1e-5 relative + 1e-6.

The native step's distances from float64 on an MI355X (largest over each group; every test prints its own before it
asserts), attention pooling at the reference dims: attn_V.weight 8.2e-7, attn_V.bias 1.3e-6, attn_U.weight 7.7e-7,
|attn_U.bias| 5.1e-9, classifier.0.weight 2.0e-7, .0.bias 2.0e-7, .2.weight 8.4e-7, .2.bias 1.2e-6, logits 4.5e-7, loss 3.3e-8
absolute; (1024,256,256,2): attn_V.weight 8.0e-7, attn_V.bias 2.4e-6, |attn_U.bias| 9.9e-10, logits 9.4e-7; (128,64,32,3):
attn_V.weight 6.9e-7, attn_V.bias 9.8e-7, |attn_U.bias| 4.7e-10; max pooling at the reference dims: .2.weight 1.8e-6 / gate
3.4e-6, .2.bias 1.6e-6 / 4.3e-6, logits 1.1e-6 / 3.6e-6.
"""
import json
import os

import numpy as np
import pytest
import torch

import mil_train_cases as cases
from ss25_hierarchical_multiscale_image_classification_amd import capi, mil, mil_train
from ss25_hierarchical_multiscale_image_classification_amd import main as cli

pytestmark = pytest.mark.gpu

UB = "aggregator.attn_U.bias"
FACTOR = 10.0
MEASURED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mil_train_fp32_distances.json")))
GATES = MEASURED["per_group"]


def gates_of(dims, pooling):
    return GATES[",".join(map(str, dims)) + "," + pooling]


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def trainer_of(model, pooling, cw=None, **kw):
    return mil_train.NativeMILTrainer(model.state_dict(), pooling, dev(), class_weights=cw, **kw)


def check(tag, dims, pooling, loss, logits, grads, ref):
    l64, z64, g64 = ref
    g = gates_of(dims, pooling)
    figures = {"loss": abs(float(loss) - float(l64)), "logits": cases.rel(logits, z64)}
    for k in g64:
        figures[k] = float(grads[k].abs().max()) if k == UB else cases.rel(grads[k], g64[k])
    print(f"[mil_train] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert figures["loss"] <= 1e-5 * abs(float(l64)) + 1e-6, (tag, figures["loss"])
    assert figures["logits"] <= FACTOR * g["logits"], (tag, "logits", figures["logits"])
    for k in g64:
        bound = FACTOR * (g["attn_U_bias_abs"] if k == UB else g[k])
        assert figures[k] <= bound, (tag, k, figures[k], bound)
    assert sorted(grads) == sorted(g64)


@pytest.mark.parametrize("cid,dims,pooling,weighted,permuted", cases.case_list(), ids=[c[0] for c in cases.case_list()])
def test_loss_logits_and_gradients_match_float64_autograd(cid, dims, pooling, weighted, permuted):
    model = cases.make_model(dims, pooling)
    feats, rows, offsets, labels, cw = cases.make_inputs(dims, permuted)
    cw = cw if weighted else None
    ref = cases.autograd_reference(model, pooling, feats, rows, offsets, labels, cw, torch.float64)
    t = trainer_of(model, pooling, cw)
    loss, logits = t.forward_backward(feats.to(dev()), rows, offsets, labels, want_attn=True)
    torch.cuda.synchronize()
    check(cid, dims, pooling, loss, logits, t.grad_dict(), ref)
    if pooling == "attention":  # the softmax weights of every bag sum to 1
        sums = torch.stack([t.attn[a:b].sum() for a, b in zip(offsets[:-1], offsets[1:])]).cpu()
        assert float((sums - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("pooling", cases.POOLINGS)
def test_two_runs_are_bitwise_equal(pooling):
    dims = cases.DIMS[0]
    model = cases.make_model(dims, pooling)
    feats, rows, offsets, labels, cw = cases.make_inputs(dims, True)
    fd = feats.to(dev())
    outs = []
    for _ in range(2):
        t = trainer_of(model, pooling, cw)
        loss, logits = t.forward_backward(fd, rows, offsets, labels)
        torch.cuda.synchronize()
        outs.append((loss.cpu(), logits.cpu(), {k: v.cpu() for k, v in t.grad_dict().items()}))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for k in outs[0][2]:
        assert torch.equal(outs[0][2][k], outs[1][2][k]), k


@pytest.mark.parametrize("pooling", cases.POOLINGS)
def test_accumulate_adds_the_gradients_of_two_batches(pooling):
    dims = cases.DIMS[0]
    model = cases.make_model(dims, pooling)
    a, b = cases.accumulate_inputs(dims)
    ra = cases.autograd_reference(model, pooling, *a, torch.float64)
    rb = cases.autograd_reference(model, pooling, *b, torch.float64)
    t = trainer_of(model, pooling, a[4])
    t.forward_backward(a[0].to(dev()), a[1], a[2], a[3])
    loss, logits = t.forward_backward(b[0].to(dev()), b[1], b[2], b[3], accumulate=True)
    torch.cuda.synchronize()
    check(f"accumulate-{pooling}", dims, pooling, loss, logits, t.grad_dict(), (rb[0], rb[1], {k: ra[2][k] + rb[2][k] for k in ra[2]}))


def test_l2_term_is_torch_adams_weight_decay():
    model = cases.make_model(cases.DIMS[0], "attention")
    t = trainer_of(model, "attention")
    torch.manual_seed(3)
    t.opt.grads.copy_(torch.randn_like(t.opt.grads))
    want = t.opt.grads.double() + 1e-4 * t.opt.params.double()
    capi._check(t.lib.hipac_mil_train_l2_add(t.opt.grads.data_ptr(), t.opt.params.data_ptr(), t.opt.params.numel(), 1e-4,
                                             capi._stream()), "l2")
    torch.cuda.synchronize()
    assert float((t.opt.grads.double() - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())  # one fp32 rounding


@pytest.mark.parametrize("pooling", cases.POOLINGS)
def test_five_steps_follow_torch_adam_on_the_float64_twin(pooling):
    """Five steps of NativeMILTrainer.step against torch.optim.Adam(lr=1e-3, weight_decay=1e-4) on the float64 twin.
    Adam divides the gradient by its own magnitude, so the figure is the error of the MOVEMENT, |p - p64|_2 / |p64 - p0|_2
    per tensor; the gate is 10 x what torch's float32 twin leaves on the same inputs
    (tests/tools/measure_mil_train_fp32.py, "adam": 6e-7 .. 3.2e-5 per tensor)."""
    model = cases.make_model(cases.DIMS[0], pooling)
    feats, rows, offsets, labels, cw = cases.adam_inputs(cases.DIMS[0])
    p64 = cases.adam_twin(model, pooling, torch.float64)
    t = trainer_of(model, pooling, cw, lr=cases.ADAM_LR, weight_decay=cases.ADAM_WD)
    fd = feats.to(dev())
    for _ in range(cases.ADAM_STEPS):
        t.step(fd, rows, offsets, labels)
    torch.cuda.synchronize()
    sd, p0 = t.state_dict(), model.state_dict()
    figures = {k: float((sd[k].cpu().double() - p64[k]).norm() / (p64[k] - p0[k].double()).norm()) for k in p64}
    print(f"[mil_train] adam-{pooling}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    for k, v in figures.items():
        assert v <= FACTOR * MEASURED["adam"][pooling][k], (k, v)


def test_step_applies_the_weight_decay():
    """The L2 term reaches the optimizer through step(): after one step the gradient buffer holds g + wd * p0, so the
    buffers of a weight_decay = 1e-4 trainer and of a weight_decay = 0 trainer differ by wd * p0 (one fp32 rounding of
    the larger buffer), and their parameters differ."""
    model = cases.make_model(cases.DIMS[0], "attention")
    feats, rows, offsets, labels, cw = cases.make_inputs(cases.DIMS[0], True, sizes=cases.SIZES[:9])
    fd = feats.to(dev())
    t0, t1 = trainer_of(model, "attention", cw, weight_decay=0.0), trainer_of(model, "attention", cw, weight_decay=1e-4)
    p0 = t1.opt.params.clone()
    t0.step(fd, rows, offsets, labels), t1.step(fd, rows, offsets, labels)
    torch.cuda.synchronize()
    want = t0.opt.grads.double() + 1e-4 * p0.double()
    assert float((t1.opt.grads.double() - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())
    assert float((t1.opt.grads - t0.opt.grads).abs().max()) > 1e-6  # wd * max|p0| ~ 4e-6: the term is there
    assert not torch.equal(t0.opt.params, t1.opt.params)


def write_triple(root, seed=0, level=2):
    rng = np.random.default_rng(seed)
    direction = rng.standard_normal(64).astype(np.float32)
    direction /= np.linalg.norm(direction)
    feats, labels, paths = [], [], []
    for b in range(60):
        n = int(rng.integers(20, 401))
        x = rng.standard_normal((n, 64)).astype(np.float32)
        lab = np.zeros(n, np.int64)
        if b % 2:
            hot = rng.choice(n, size=max(3, n // 10), replace=False)
            x[hot] += 4.0 * direction
            lab[hot] = 1
        feats.append(x), labels.append(lab)
        paths += [f"slide{b}/slide{b}_x{b}_y{i}_{'tumor' if l else 'normal'}.png" for i, l in enumerate(lab)]
    names = (os.path.join(root, f"patch_features_{level}.npy"), os.path.join(root, f"patch_labels_{level}.npy"),
             os.path.join(root, f"patch_paths_{level}.txt"))
    np.save(names[0], np.concatenate(feats)), np.save(names[1], np.concatenate(labels))
    with open(names[2], "w") as f:
        f.write("\n".join(paths) + "\n")
    return names


def twin_train(names, pooling, epochs, seed, patience=5):
    """train_mil's loop on the float64 twin: the same split, batches, early-stopping rule; -> test accuracy."""
    feats, order, offsets, bag_names, wsi = mil_train.load_triple(*names)
    tr, va, te = mil_train.split_bags(len(bag_names), seed)
    m = mil.MILClassifier(feats.shape[1], 2, pooling)
    m.load_state_dict(mil_train.initial_state_dict(feats.shape[1], pooling, seed))
    m = m.double().train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    x, y = torch.from_numpy(feats).double(), torch.from_numpy(wsi)
    bag = lambda b: x[order[offsets[b]:offsets[b + 1]]]
    best, best_sd, bad = float("inf"), None, 0
    import copy
    for epoch in range(epochs):
        for rows, offs, group in mil_train.epoch_batches(tr, order, offsets, epoch, seed, 32, None):
            opt.zero_grad()
            logits = torch.stack([m(x[rows[a:b]])[0] for a, b in zip(offs[:-1], offs[1:])])
            torch.nn.functional.cross_entropy(logits, y[group]).backward()
            opt.step()
        with torch.no_grad():
            v = float(torch.nn.functional.cross_entropy(torch.stack([m(bag(b))[0] for b in va]), y[va]))
        if v < best:
            best, best_sd, bad = v, copy.deepcopy(m.state_dict()), 0
        else:
            bad += 1
        if bad >= patience:
            break
    m.load_state_dict(best_sd)
    with torch.no_grad():
        pred = torch.stack([m(bag(b))[0] for b in te]).argmax(1).numpy()
    return float((pred == wsi[te]).mean()), len(te)


def test_train_mil_end_to_end_and_cli(tmp_path, monkeypatch):
    names = write_triple(str(tmp_path))
    out = str(tmp_path / "run")
    metrics = mil_train.train_mil(*names, epochs=12, seed=0, out_dir=out)
    assert metrics["train_loss"][-1] < metrics["train_loss"][0]
    assert metrics["early_stopped"] or metrics["epochs_run"] == 12
    assert metrics["split_sizes"] == {"train": 48, "val": 6, "test": 6}
    for k in ("accuracy", "precision", "recall", "f1_score", "confusion_matrix", "train_loss", "val_loss"):
        assert k in metrics
    assert json.load(open(os.path.join(out, "results", "metrics.json")))["accuracy"] == metrics["accuracy"]
    sd = torch.load(os.path.join(out, "models", "mil_model.pth"), map_location="cpu", weights_only=True)
    mil.MILClassifier(64, 2, "attention").load_state_dict(sd, strict=True)
    acc64, n_test = twin_train(names, "attention", 12, 0)
    print(f"[mil_train] end to end: native test accuracy {metrics['accuracy']:.4f}, float64 twin {acc64:.4f} ({n_test} test bags)")
    assert abs(metrics["accuracy"] - acc64) <= 1.0 / n_test + 1e-12
    monkeypatch.chdir(tmp_path)
    assert cli.main(["--train_mil", "--patch_level", "2", "--mil_epochs", "2", "--seed", "0"]) == 0
    assert os.path.exists("models/mil_model.pth") and os.path.exists("results/metrics.json")
    assert cli.main(["--predict_mil", "--patch_level", "2"]) == 0
    lines = open("results/mil_predictions.csv").read().strip().split("\n")
    assert lines[0] == "bag,probability,prediction" and len(lines) == 61
    assert cli.main(["--train_mil", "--patch_level", "2", "--mil_pooling", "max", "--mil_bag_size", "100", "--max_steps", "3"]) == 0


def test_error_paths():
    dims = cases.DIMS[0]
    model = cases.make_model(dims, "attention")
    t = trainer_of(model, "attention")
    feats = torch.randn(100, 512)
    fd = feats.to(dev())
    lab = torch.tensor([0, 1])
    with pytest.raises(capi.HipacError):  # empty bag
        t.forward_backward(fd, None, [0, 50, 50, 100], torch.tensor([0, 1, 0]))
    with pytest.raises(capi.HipacError):  # offsets not covering n
        t.forward_backward(fd, None, [0, 50, 90], lab)
    with pytest.raises(capi.HipacError):
        t.forward_backward(fd, torch.arange(80), [0, 50, 90], lab)
    with pytest.raises(capi.HipacError):  # a row index outside [0, N): refused on the host
        t.forward_backward(fd, torch.tensor([0, 5, 100]), [0, 2, 3], lab)
    with pytest.raises(capi.HipacError):
        t.forward_backward(fd, torch.tensor([0, -1, 7]), [0, 2, 3], lab)
    with pytest.raises(capi.HipacError):  # CPU tensor
        t.forward_backward(feats, None, [0, 50, 100], lab)
    with pytest.raises(capi.HipacError):  # float64 features
        t.forward_backward(fd.double(), None, [0, 50, 100], lab)
    with pytest.raises(capi.HipacError):  # a label outside [0, C)
        t.forward_backward(fd, None, [0, 50, 100], torch.tensor([0, 2]))
    loss, logits = t.forward_backward(fd, None, [0, 50, 100], lab)  # and the trainer still works afterwards
    assert logits.shape == (2, 2) and bool(torch.isfinite(loss))
