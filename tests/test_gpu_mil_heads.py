"""Multi-head attention pooling on the device (csrc/mil_heads.hip, include/hipac_mil_heads.h): the training step
(mil_train.NativeMILTrainer on a K-head model) and the inference forward (MILClassifier.eval() / forward_bags) against the
plain-torch twin of tests/mil_heads_cases.py in float64 on the CPU -- never against the native forward.

Tolerances: the rule and the factor of tests/test_gpu_mil_train.py.  Each tensor is gated at 10 x the distance torch's OWN
float32 autograd keeps from its float64 autograd on exactly these inputs, metric max|a - b| / max|b|, measured on the CPU
by tests/tools/measure_mil_heads_fp32.py and kept in tests/golden/mil_heads_fp32_distances.json.  A gate is formed over the
cases that run the same computation -- the same (F, A, hidden, C, K) -- and takes the largest of their figures; nothing is
pooled across dims.  aggregator.attn_U.bias (K values) has gradient 0 in exact arithmetic and is gated absolutely at 10 x
what float32 autograd leaves there.  Loss: 1e-5 relative + 1e-6.  Measured fp32-vs-fp64 (x 10 = the gate):

    (512,128,128,2,8):  attn_V.weight 3.3e-7  attn_V.bias 1.3e-6  attn_U.weight 4.5e-7  |attn_U.bias| 9.1e-10  classifier.0.weight 2.1e-7
                        .0.bias 1.3e-7  .2.weight 4.0e-7  .2.bias 4.1e-6  logits 5.2e-7  attn 4.8e-8
    (128,64,32,3,3):    attn_V.weight 2.0e-7  attn_V.bias 3.4e-7  attn_U.weight 2.6e-7  |attn_U.bias| 6.3e-10  logits 1.7e-7  attn 2.9e-8
    (1024,256,256,2,2): attn_V.weight 3.6e-7  attn_V.bias 8.1e-7  attn_U.weight 3.3e-7  |attn_U.bias| 1.2e-9   logits 1.1e-7  attn 3.9e-8
    (512,128,128,2,1):  attn_V.weight 1.1e-6  attn_V.bias 1.2e-6  attn_U.weight 8.3e-7  |attn_U.bias| 3.6e-10  logits 1.8e-7  attn 1.7e-8
    forward without gradients: logits 1.3e-7 .. 6.3e-7, attn 2.0e-8 .. 4.8e-8, pooled 5.1e-8 .. 6.3e-8 (see the json)

The native figures on an MI355X (largest over each group; every test prints its own before it asserts):
    (512,128,128,2,8), the accumulate case included: attn_V.weight 6.7e-7, attn_V.bias 1.5e-6, attn_U.weight 5.4e-7, |attn_U.bias| 1.9e-9,
        classifier.0.weight 2.8e-7, .0.bias 2.0e-7, .2.weight 3.1e-6 / gate 4.0e-6, .2.bias 5.4e-6 / 4.1e-5, logits 2.3e-6 / 5.2e-6,
        attn 5.8e-8, loss 6.7e-8 absolute
    (128,64,32,3,3): attn_V.weight 3.8e-7, attn_V.bias 1.0e-6, attn_U.weight 3.7e-7, |attn_U.bias| 1.7e-9 / 6.3e-9, logits 2.4e-7, attn 6.0e-8
    (1024,256,256,2,2): attn_V.weight 7.5e-7, attn_V.bias 2.2e-6, attn_U.weight 1.1e-6 / 3.3e-6, |attn_U.bias| 3.6e-10, logits 6.5e-7 / 1.1e-6
    (512,128,128,2,1), the new entry point: attn_V.weight 1.1e-6, attn_V.bias 2.3e-6, attn_U.weight 9.9e-7, |attn_U.bias| 2.9e-9 / 3.6e-9,
        logits 1.3e-7
    forward without gradients: logits 2.3e-6 / 6.3e-6, 7.0e-7 / 3.1e-6, 3.3e-7 / 1.5e-6, 3.1e-7 / 1.3e-6 in the order above;
        attn <= 4.8e-8, pooled <= 6.3e-8; attention column sums within 1.8e-7 of 1
"""
import json
import os

import numpy as np
import pytest
import torch

import mil_heads_cases as cases
from ss25_hierarchical_multiscale_image_classification_amd import capi, mil, mil_heads, mil_train
from ss25_hierarchical_multiscale_image_classification_amd import main as cli

pytestmark = pytest.mark.gpu

UB = "aggregator.attn_U.bias"
FACTOR = 10.0
MEASURED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mil_heads_fp32_distances.json")))
CASES = cases.case_list()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def trainer_of(twin, cw=None, **kw):
    return mil_train.NativeMILTrainer(twin.state_dict(), "attention", dev(), class_weights=cw, **kw)


_refs = {}


def reference(cid, dims, weighted, permuted):
    """The float64 twin's step for a case, computed once and shared."""
    if cid not in _refs:
        twin = cases.make_twin(dims)
        feats, rows, offsets, labels, cw = cases.make_inputs(dims, permuted)
        cw = cw if weighted else None
        _refs[cid] = (twin, (feats, rows, offsets, labels, cw), cases.reference(twin, feats, rows, offsets, labels, cw, torch.float64))
    return _refs[cid]


def check(tag, dims, loss, logits, attn, grads, ref):
    l64, z64, a64, g64 = ref
    g = MEASURED["per_group"][cases.group_key(dims)]
    figures = {"loss": abs(float(loss) - float(l64)), "logits": cases.rel(logits, z64)}
    if attn is not None:
        figures["attn"] = cases.rel(attn, a64)
    for k in g64:
        figures[k] = float(grads[k].abs().max()) if k == UB else cases.rel(grads[k], g64[k])
    print(f"[mil_heads] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert sorted(grads) == sorted(g64)
    assert figures["loss"] <= 1e-5 * abs(float(l64)) + 1e-6, (tag, figures["loss"])
    assert figures["logits"] <= FACTOR * g["logits"], (tag, "logits", figures["logits"])
    if attn is not None:
        assert figures["attn"] <= FACTOR * g["attn"], (tag, "attn", figures["attn"], FACTOR * g["attn"])
    for k in g64:
        bound = FACTOR * (g["attn_U_bias_abs"] if k == UB else g[k])
        assert figures[k] <= bound, (tag, k, figures[k], bound)


@pytest.mark.parametrize("cid,dims,weighted,permuted", CASES, ids=[c[0] for c in CASES])
def test_step_matches_the_float64_twin(cid, dims, weighted, permuted):
    K = dims[4]
    twin, (feats, rows, offsets, labels, cw), ref = reference(cid, dims, weighted, permuted)
    t = trainer_of(twin, cw)
    assert t.heads == K
    if K == 1:  # heads = 1 through the NEW entry point (the trainer itself sends one head through the old one)
        loss, logits, attn, grads = direct_heads_step(t, feats.to(dev()), rows, offsets, labels, 1)
    else:
        loss, logits = t.forward_backward(feats.to(dev()), rows, offsets, labels, want_attn=True)
        attn, grads = t.attn, t.grad_dict()
    torch.cuda.synchronize()
    assert attn.shape == (int(offsets[-1]), K)
    check(cid, dims, loss, logits, attn, grads, ref)
    sums = torch.stack([attn[a:b].sum(0) for a, b in zip(offsets[:-1], offsets[1:])]).cpu()  # per bag and head
    print(f"[mil_heads] {cid}: attention column sums within {float((sums - 1).abs().max()):.2e} of 1")
    assert sums.shape == (len(offsets) - 1, K) and float((sums - 1).abs().max()) < 1e-5


def direct_heads_step(t, feats, rows, offsets, labels, heads, accumulate=False):
    """hipac_mil_heads_train_fwd_bwd called directly on the trainer's buffers."""
    import ctypes as C

    lib = mil_heads.load_mil_heads_library()
    n, B = int(offsets[-1]), len(offsets) - 1
    need = lib.hipac_mil_heads_train_workspace_bytes(C.addressof(t._p), heads, n, B)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    rows_dev = None if rows is None else rows.to(dev(), torch.int32)
    offs = torch.from_numpy(np.asarray(offsets).astype(np.int32)).to(dev())
    lab = labels.to(dev())
    loss = torch.empty((), dtype=torch.float32, device=dev())
    logits = torch.empty((B, t.C), dtype=torch.float32, device=dev())
    attn = torch.empty((n, heads), dtype=torch.float32, device=dev())
    rc = lib.hipac_mil_heads_train_fwd_bwd(C.addressof(t._p), heads, feats.data_ptr(), feats.shape[0], capi._ptr(rows_dev),
                                           offs.data_ptr(), n, B, lab.data_ptr(), capi._ptr(t.class_weights), C.addressof(t._g),
                                           loss.data_ptr(), logits.data_ptr(), attn.data_ptr(), ws.data_ptr(), ws.numel(),
                                           1 if accumulate else 0, capi._stream())
    capi._check(rc, "hipac_mil_heads_train_fwd_bwd")
    torch.cuda.synchronize()
    return loss, logits, attn, t.grad_dict()


@pytest.mark.parametrize("dims", cases.DIMS, ids=[cases.group_key(d) for d in cases.DIMS])
def test_inference_forward_matches_the_float64_twin(dims):
    F, A, hidden, C, K = dims
    twin = cases.make_twin(dims)
    feats, _, offsets, _, _ = cases.make_inputs(dims, False)
    z64, a64, p64 = cases.eval_reference(twin, feats, offsets, torch.float64)
    g = MEASURED["eval"][cases.group_key(dims)]
    fd = feats.to(dev())
    if K == 1:  # heads = 1 through the NEW entry point (MILClassifier sends one head through hipac_mil_forward)
        sd = {k: v.detach().to(dev()).contiguous() for k, v in twin.state_dict().items()}
        logits, attn, pooled = mil_heads.heads_forward(sd, fd, offsets, want_pooled=True)
    else:
        model = mil.MILClassifier(F, C, "attention", heads=K, attn_dim=A, hidden_dim=hidden)
        model.load_state_dict(twin.state_dict(), strict=True)
        model = model.to(dev()).eval()
        logits, attn, pooled = model.forward_bags(fd, offsets, want_pooled=True)
        one_logits, one_attn = model(fd[offsets[3]:offsets[4]])  # forward() of one bag: the same entry point
        torch.cuda.synchronize()
        assert one_attn.shape == (offsets[4] - offsets[3], K) and one_logits.shape == (C,)
        assert cases.rel(one_logits, z64[3]) <= FACTOR * g["logits"] * float(z64.abs().max() / z64[3].abs().max())
    torch.cuda.synchronize()
    assert logits.shape == (len(offsets) - 1, C) and attn.shape == (feats.shape[0], K) and pooled.shape == (len(offsets) - 1, K * F)
    figures = {"logits": cases.rel(logits, z64), "attn": cases.rel(attn, a64), "pooled": cases.rel(pooled, p64)}
    print(f"[mil_heads] eval {dims}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    for k, v in figures.items():
        assert v <= FACTOR * g[k], (k, v, FACTOR * g[k])


def test_two_runs_are_bitwise_equal():
    cid, dims, weighted, permuted = CASES[3]  # the reference dims, K = 8, weighted, permuted
    twin, (feats, rows, offsets, labels, cw), _ = reference(cid, dims, weighted, permuted)
    fd = feats.to(dev())
    outs = []
    for _ in range(2):
        t = trainer_of(twin, cw)
        loss, logits = t.forward_backward(fd, rows, offsets, labels, want_attn=True)
        torch.cuda.synchronize()
        outs.append((loss.cpu(), logits.cpu(), t.attn.cpu(), {k: v.cpu() for k, v in t.grad_dict().items()}))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    for k in outs[0][3]:
        assert torch.equal(outs[0][3][k], outs[1][3][k]), k


def test_accumulate_adds_the_gradients_of_two_batches():
    dims = cases.DIMS[0]
    twin = cases.make_twin(dims)
    a, b = cases.accumulate_inputs(dims)
    ra, rb = cases.reference(twin, *a, torch.float64), cases.reference(twin, *b, torch.float64)
    t = trainer_of(twin, a[4])
    t.forward_backward(a[0].to(dev()), a[1], a[2], a[3])
    loss, logits = t.forward_backward(b[0].to(dev()), b[1], b[2], b[3], accumulate=True)
    torch.cuda.synchronize()
    check("accumulate", dims, loss, logits, None, t.grad_dict(), (rb[0], rb[1], None, {k: ra[3][k] + rb[3][k] for k in ra[3]}))


def test_one_head_trainer_still_takes_the_old_entry_point():
    """A heads == 1 trainer built by the public API against a direct hipac_mil_train_fwd_bwd call on the same inputs:
    bit-identical loss, logits, gradients."""
    import ctypes as C

    dims = cases.DIMS[3]
    twin = cases.make_twin(dims)
    model = mil.MILClassifier(dims[0], dims[3], "attention", heads=1)
    model.load_state_dict(twin.state_dict(), strict=True)
    feats, rows, offsets, labels, cw = cases.make_inputs(dims, True)
    fd = feats.to(dev())
    t = mil_train.NativeMILTrainer(model.state_dict(), "attention", dev(), class_weights=cw)
    assert t.heads == 1
    loss, logits = t.forward_backward(fd, rows, offsets, labels, want_attn=True)
    torch.cuda.synchronize()
    assert t.attn.shape == (int(offsets[-1]),)
    got = (loss.cpu(), logits.cpu(), t.attn.cpu(), {k: v.cpu() for k, v in t.grad_dict().items()})
    d = mil_train.NativeMILTrainer(twin.state_dict(), "attention", dev(), class_weights=cw)
    lib = mil_train.load_mil_train_library()
    n, B = int(offsets[-1]), len(offsets) - 1
    need = lib.hipac_mil_train_workspace_bytes(C.addressof(d._p), 0, n, B)
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    rows_dev, offs, lab = rows.to(dev(), torch.int32), torch.from_numpy(offsets.astype(np.int32)).to(dev()), labels.to(dev())
    loss2, logits2 = torch.empty((), device=dev()), torch.empty((B, dims[3]), device=dev())
    attn2 = torch.empty(n, device=dev())
    capi._check(lib.hipac_mil_train_fwd_bwd(C.addressof(d._p), 0, fd.data_ptr(), fd.shape[0], rows_dev.data_ptr(), offs.data_ptr(), n, B,
                                            lab.data_ptr(), d.class_weights.data_ptr(), C.addressof(d._g), loss2.data_ptr(),
                                            logits2.data_ptr(), attn2.data_ptr(), ws.data_ptr(), ws.numel(), 0, capi._stream()),
                "hipac_mil_train_fwd_bwd")
    torch.cuda.synchronize()
    assert torch.equal(got[0], loss2.cpu()) and torch.equal(got[1], logits2.cpu()) and torch.equal(got[2], attn2.cpu())
    want = d.grad_dict()
    for k in want:
        assert torch.equal(got[3][k], want[k].cpu()), k


def test_one_head_eval_is_mil_forward():
    dims = cases.DIMS[3]
    model = mil.MILClassifier(dims[0], dims[3], "attention", heads=1)
    model.load_state_dict(cases.make_twin(dims).state_dict(), strict=True)
    model = model.to(dev()).eval()
    feats, _, offsets, _, _ = cases.make_inputs(dims, False)
    fd = feats.to(dev())
    logits, attn, pooled = model.forward_bags(fd, offsets, want_pooled=True)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    l2, a2, p2 = capi.mil_forward(sd, "attention", fd, torch.from_numpy(offsets), want_pooled=True)
    torch.cuda.synchronize()
    assert attn.shape == (feats.shape[0],)
    assert torch.equal(logits, l2) and torch.equal(attn, a2) and torch.equal(pooled, p2)
    z, a = model(fd[offsets[5]:offsets[6]])
    assert a.shape == (offsets[6] - offsets[5], 1)


def write_triple(root, level=2, seed=0):
    """12 bags of about 40 rows, F = 512; the odd bags carry rows shifted along one direction (separable classes).  The rows
    of the bags are interleaved in the files, so the file order is not the bag order."""
    rng = np.random.default_rng(seed)
    direction = rng.standard_normal(512).astype(np.float32)
    direction /= np.linalg.norm(direction)
    rows = []
    for b in range(12):
        n = int(rng.integers(35, 46))
        x = rng.standard_normal((n, 512)).astype(np.float32)
        lab = np.zeros(n, np.int64)
        if b % 2:
            hot = rng.choice(n, size=6, replace=False)
            x[hot] += 6.0 * direction
            lab[hot] = 1
        rows += [(x[i], lab[i], f"slide{b}/slide{b}_x{b}_y{i}_{'tumor' if lab[i] else 'normal'}.png") for i in range(n)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    names = (os.path.join(root, f"patch_features_{level}.npy"), os.path.join(root, f"patch_labels_{level}.npy"),
             os.path.join(root, f"patch_paths_{level}.txt"))
    np.save(names[0], np.stack([r[0] for r in rows])), np.save(names[1], np.array([r[1] for r in rows]))
    with open(names[2], "w") as f:
        f.write("\n".join(r[2] for r in rows) + "\n")
    return names, [r[2] for r in rows]


def bag_sums(attention, paths):
    keys = ["_".join(os.path.basename(p).split("_")[:-2]) for p in paths]
    return np.stack([attention[[i for i, k in enumerate(keys) if k == key]].sum(0) for key in dict.fromkeys(keys)])


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_end_to_end_cli(tmp_path, monkeypatch):
    names, paths = write_triple(str(tmp_path))
    n = len(paths)
    monkeypatch.chdir(tmp_path)
    train4 = ["--train_mil", "--patch_level", "2", "--mil_heads", "4", "--mil_epochs", "3", "--seed", "0"]
    assert cli.main(train4) == 0
    first = read("models/mil_model.pth")
    sd = torch.load("models/mil_model.pth", map_location="cpu", weights_only=True)
    assert tuple(sd["aggregator.attn_U.weight"].shape) == (4, 128) and tuple(sd["classifier.0.weight"].shape) == (128, 2048)
    metrics = json.load(open("results/metrics.json"))
    assert metrics["attention_heads"] == 4 and metrics["train_loss"][-1] < metrics["train_loss"][0]
    assert cli.main(["--predict_mil", "--patch_level", "2", "--mil_save_attention"]) == 0  # K comes from the model
    lines = read("results/mil_predictions.csv").decode().strip().split("\n")
    assert lines[0] == "bag,probability,prediction" and len(lines) == 13
    att = np.load("results/mil_attention.npy")
    assert att.shape == (n, 4) and att.dtype == np.float32
    sums = bag_sums(att, paths)  # grouped by the triple's own path lines: the row order is the triple's
    assert sums.shape == (12, 4) and float(np.abs(sums - 1).max()) < 1e-5
    assert cli.main(["--predict_mil", "--patch_level", "2", "--mil_heads", "2"]) == 2  # disagrees with the model
    assert cli.main(train4) == 0  # two identical runs: byte-identical model files
    assert read("models/mil_model.pth") == first

    # one head: the files the old path writes
    assert cli.main(["--train_mil", "--patch_level", "2", "--mil_heads", "1", "--mil_epochs", "3", "--seed", "0"]) == 0
    model1, metrics1 = read("models/mil_model.pth"), json.load(open("results/metrics.json"))
    assert "attention_heads" not in metrics1
    assert cli.main(["--predict_mil", "--patch_level", "2", "--mil_heads", "1", "--mil_save_attention"]) == 0
    csv1, att1 = read("results/mil_predictions.csv"), np.load("results/mil_attention.npy")
    assert att1.shape == (n, 1) and float(np.abs(bag_sums(att1, paths) - 1).max()) < 1e-5
    out = str(tmp_path / "api")
    api_metrics = mil_train.train_mil(*names, epochs=3, seed=0, out_dir=out, heads=1)
    assert read(os.path.join(out, "models", "mil_model.pth")) == model1
    assert api_metrics == metrics1
    # ... and the attention file is hipac_mil_forward's own attention output, row for row
    mil_train.predict_mil(os.path.join(out, "models", "mil_model.pth"), *names, out_dir=out)
    assert read(os.path.join(out, "results", "mil_predictions.csv")) == csv1
    feats, order, offsets, _, _ = mil_train.load_triple(*names)
    sd1 = {k: v.to(dev()) for k, v in torch.load("models/mil_model.pth", map_location="cpu", weights_only=True).items()}
    _, a, _ = capi.mil_forward(sd1, "attention", torch.from_numpy(feats[order]).to(dev()), torch.from_numpy(offsets))
    want = np.empty(n, np.float32)
    want[order] = a.cpu().numpy()
    assert np.array_equal(att1[:, 0], want)
