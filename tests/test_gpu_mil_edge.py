"""The single-head MIL head at the edges of its dims against float64 on the CPU: the native training step
(csrc/mil_train.hip through mil_train.NativeMILTrainer.forward_backward) against torch autograd in float64, the inference
head (csrc/mil.hip through mil.MILClassifier.forward_bags / forward) against a float64 restatement.  The cases, references,
metrics and gates are those of tests/mil_edge_cases.py, whose docstring says what each shape reaches;
tests/test_oracle_mil_edge.py shows on the CPU that they notice the faults a kernel could have.

Gates: every figure at 10 x the distance torch's own float32 CPU computation keeps from the float64 reference on exactly
these inputs, the largest over the cases of a group (train / infer, dims, pooling, kind), from
tests/golden/mil_edge_fp32_distances.json (tests/tools/measure_mil_edge_fp32.py).  The largest measured float32 figure is
2.0e-5 (attn_V.weight of (2048,31,17,2) peaked), so no gate exceeds 2.0e-4.  Every test prints its figures next to the gates
before it asserts.

Measured on an MI355X, the largest figure over each group / its gate ("grads": the gradient figure, rel or row_rel, closest
to its gate, with the bag sizes of the case that gave it; |db_U| is max|d attn_U.bias|, gated absolutely):

    training step, attention pooling
    (4,1,3,2)        plain   logits 7.6e-8 / 8.6e-7   attn 5.7e-8 / 5.4e-7   |db_U| 3.0e-9 / 6.4e-9    grads attn_V.bias 2.4e-5 / 8.7e-5 (mix)
                     peaked  logits 3.2e-7 / 3.3e-6   attn 1.6e-6 / 1.6e-5   |db_U| 1.4e-9 / 1.5e-7    grads attn_V.weight 2.8e-6 / 2.4e-5 (mix)
    (36,33,5,3)      plain   logits 1.5e-7 / 1.5e-6   attn 6.2e-8 / 6.2e-7   |db_U| 5.2e-10 / 4.2e-8   grads row .2.weight 4.4e-7 / 3.1e-6 (pair)
                     peaked  logits 7.7e-7 / 7.7e-6   attn 1.4e-6 / 1.5e-5   |db_U| 7.6e-11 / 3.0e-8   grads attn_V.bias 2.9e-6 / 3.5e-5 (tile)
    (68,65,255,16)   plain   logits 3.6e-7 / 2.4e-6   attn 6.8e-8 / 5.6e-7   |db_U| 6.7e-10 / 2.6e-8   grads row .2.weight 7.5e-7 / 5.0e-6 (many)
                     peaked  logits 1.0e-6 / 1.1e-5   attn 1.2e-6 / 1.1e-5   |db_U| 5.1e-10 / 1.4e-7   grads .2.weight 1.7e-6 / 6.3e-6 (tile)
    (100,250,256,2)  plain   logits 4.2e-7 / 1.8e-6   attn 5.9e-8 / 5.6e-7   |db_U| 4.7e-10 / 1.9e-8   grads row .0.weight 6.4e-6 / 4.6e-5 (mix)
                     peaked  logits 1.2e-6 / 1.0e-5   attn 1.2e-6 / 1.2e-5   |db_U| 1.7e-10 / 3.9e-8   grads .2.weight 2.1e-6 / 1.0e-5 (tile)
    (2048,31,17,2)   plain   logits 1.0e-6 / 2.0e-6   attn 1.7e-7 / 6.9e-7   |db_U| 2.3e-10 / 1.3e-8   grads .2.bias 9.3e-6 / 1.6e-5 (mix)
                     peaked  logits 2.5e-6 / 2.5e-5   attn 4.7e-6 / 2.0e-5   |db_U| 6.0e-10 / 8.5e-8   grads .2.bias 2.4e-6 / 3.8e-6 (mix)
    training step, mean / max pooling (plain): logits 8.7e-8 .. 1.7e-6 against gates 9.8e-7 .. 4.8e-6; the gradient closest to its
                     gate is .2.weight of (2048,31,17,2) max, 3.3e-6 / 9.9e-6 (big).  Loss: at most 3.5e-7 absolute, gates 5e-6 .. 3e-5.
    ``one`` under attention pooling: attn is 1.0 and all four attention gradients are exactly 0 at every dims (the derived bound
                     allows up to 2 (F + 2) 2^-24 sum|x g|); C = 1: loss 0 and every gradient exactly 0 under all three poolings.
    inference head, attention pooling: plain  logits 1.4e-7 .. 2.0e-6 / 1.3e-6 .. 4.9e-6, attn 5.6e-8 .. 1.1e-7 / 5.4e-7 .. 6.9e-7,
                     pooled 5.6e-8 .. 1.2e-7 / 6.7e-7 .. 1.0e-6; peaked  logits 6.3e-7 .. 1.5e-6 / 6.3e-6 .. 4.0e-5, attn 1.5e-6 .. 2.4e-6 /
                     1.2e-5 .. 2.4e-5, pooled 9.9e-7 .. 2.7e-6 / 9.9e-6 .. 3.1e-5 (the closest: logits of (4,1,3,2) and (36,33,5,3) peaked, at
                     their gates' tenth, i.e. where torch's float32 is).  mean: logits 6.9e-8 .. 1.4e-6 / 5.0e-7 .. 7.9e-6, pooled 4.3e-8 ..
                     7.2e-8 / 2.4e-7 .. 5.8e-7.  max: pooled exact (gate 0), logits 6.5e-8 .. 1.4e-6 / 5.5e-7 .. 1.1e-5.

What these tests found in the step, fixed together with them (csrc/mil_train.hip).  In exact arithmetic sum_i ds_i = 0 inside
every bag; db_U is that sum, and with A = 1 db_V = U sum_i ds_i (1 - H_i^2) is the same sum cancelled down (max|db_V| = 3.9e-5 next
to max|dV| = 1.2e-2 at (4,1,3,2) ``mix``).  The step formed ds_i = a_i (x_i . g_b - cdot_b) with cdot_b = pooled_b . g_b, a second,
independent evaluation, so the sum kept a rounding of the dot products themselves, where torch's softmax backward, which forms
both terms from ONE evaluation t_i = x_i . g_b, keeps none.  On the device that gave, against the gates above: a bag of one row
with ds_i = 1e-8 where it is exactly 0, which reached every attention gradient (attn_V.bias of (2048,31,17,2) ``pair`` 2.8e-5 / 1.6e-5,
attn_V.weight of (36,33,5,3) ``pair`` peaked 4.5e-5 / 3.5e-5, |db_U| of (2048,31,17,2) ``pair`` 2.1e-8 / 1.3e-8), and at (4,1,3,2) ``mix``
attn_V.bias 9.4e-5 / 8.7e-5 and |db_U| 6.7e-9 / 6.4e-9 (one ulp of |t_i| ~ 0.1 is 7.5e-9).  The step now keeps the row dot products,
takes c_b = sum_j a_j t_j / sum_j a_j per bag in double and ds_i = a_i (t_i - c_b), and adds the ds sweep's column sums in double:
single-row bags are exactly 0 and |db_U| is where torch's float32 leaves it, as the table shows.
"""
import copy

import pytest
import torch

import mil_edge_cases as cases
import mil_train_cases as base
from ss25_hierarchical_multiscale_image_classification_amd import capi, mil, mil_train

pytestmark = pytest.mark.gpu

TRAIN_CASES = cases.train_cases() + [cases.ACC_CASE]
INFER_CASES = cases.infer_cases()


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def cpu(t):
    return None if t is None else t.detach().cpu()


def native_step(case):
    """(loss, logits, gradients, attn) of the native step on a train / acc case, on the CPU."""
    s = cases.setup(case)
    batches = s[1:]
    t = mil_train.NativeMILTrainer(s[0].state_dict(), case.pooling, dev(), class_weights=batches[0][4])
    for i, (feats, rows, offsets, labels, _) in enumerate(batches):
        loss, logits = t.forward_backward(feats.to(dev()), rows, offsets, labels, accumulate=i > 0, want_attn=True)
    torch.cuda.synchronize()
    return cpu(loss), cpu(logits), {k: cpu(v) for k, v in t.grad_dict().items()}, cpu(t.attn)


def native_model(case):
    return copy.deepcopy(cases.setup(case)[0]).to(dev()).eval()


@pytest.mark.parametrize("case", TRAIN_CASES, ids=[c.id for c in TRAIN_CASES])
def test_training_step_matches_float64_autograd(case):
    """Loss, logits, every gradient (rel, and row_rel where it applies) and the softmax weights against float64."""
    got = native_step(case)
    assert (got[3] is None) == (case.pooling != "attention")
    bad = cases.failures(case, got)
    assert bad == [], (case.id, bad)


def test_two_runs_at_padded_dims_are_bitwise_equal():
    """mil_train.hip promises "no float atomics": the result depends on the tiling, never on the run -- at A_pad != A, odd nAt
    and a partial second column block of mt_dv too."""
    a, b = native_step(cases.BITWISE_CASE), native_step(cases.BITWISE_CASE)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize("case", INFER_CASES, ids=[c.id for c in INFER_CASES])
def test_inference_head_matches_float64(case):
    _, x, offsets = cases.setup(case)
    logits, attn, pooled = native_model(case).forward_bags(x.to(dev()), offsets, want_pooled=True)
    torch.cuda.synchronize()
    assert (attn is None) == (case.pooling != "attention")
    bad = cases.failures(case, (cpu(logits), cpu(attn), cpu(pooled)))
    assert bad == [], (case.id, bad)


def test_single_bag_forward_matches_float64():
    """MILClassifier.forward, the reference's call shape, on the 130-row bag of ``mix`` at (68, 65, 255, 16)."""
    case = next(c for c in INFER_CASES if c.dims == cases.ACC_DIMS and c.pooling == "attention" and c.sizes == "mix" and c.kind == "plain")
    _, x, offsets = cases.setup(case)
    b = cases.SIZES["mix"].index(130)
    lo, hi = int(offsets[b]), int(offsets[b + 1])
    logits, attn = native_model(case)(x[lo:hi].to(dev()))
    torch.cuda.synchronize()
    z64, a64, _ = cases.reference(case)
    assert logits.shape == (16,) and attn.shape == (130, 1)
    # the maxima of the whole batch's tensors, as in the group's own metric
    figs = {"logits": float((cpu(logits).double() - z64[b]).abs().max() / z64.abs().max()),
            "attn": float((cpu(attn).double()[:, 0] - a64[lo:hi]).abs().max() / a64.abs().max())}
    for k, v in figs.items():
        print(f"[mil_edge] single bag: {k} {v:.2e} / gate {cases.gate(case, k):.2e}")
        assert v <= cases.gate(case, k), (k, v)


# dims outside the kernels' limits: F > 2048, F not a multiple of 4, attn_dim > 256, hidden_dim > 256, C > 16
REFUSED = [(2052, 33, 5, 2), (6, 33, 5, 2), (36, 257, 5, 2), (36, 33, 257, 2), (36, 33, 5, 17)]
GOOD = (36, 33, 5, 3)


def _small_batch(F, C):
    g = torch.Generator().manual_seed(7)
    return torch.randn(8, F, generator=g), [0, 3, 8], torch.tensor([0, C - 1])


def test_training_step_refuses_dims_outside_its_limits():
    feats, offsets, labels = _small_batch(GOOD[0], GOOD[3])
    good = mil_train.NativeMILTrainer(base.make_model(GOOD, "attention").state_dict(), "attention", dev())

    def run_good():
        loss, logits = good.forward_backward(feats.to(dev()), None, offsets, labels)
        torch.cuda.synchronize()
        return [cpu(loss), cpu(logits)] + [cpu(v) for v in good.grad_dict().values()]

    before = run_good()
    for dims in REFUSED:
        for pooling in ("attention", "mean"):
            if pooling == "mean" and dims[1] > 256:
                continue  # attn_dim does not exist there
            x, offs, lab = _small_batch(dims[0], dims[3])
            with pytest.raises(capi.HipacError):
                t = mil_train.NativeMILTrainer(base.make_model(dims, pooling).state_dict(), pooling, dev())
                t.forward_backward(x.to(dev()), None, offs, lab)
            after = run_good()  # the library and a trainer made before the refusal work as they did
            assert all(torch.equal(p, q) for p, q in zip(before, after)), (dims, pooling)


def test_inference_head_refuses_dims_outside_its_limits():
    feats, offsets, _ = _small_batch(GOOD[0], GOOD[3])
    torch.manual_seed(0)
    good = mil.MILClassifier(GOOD[0], GOOD[3], "attention", attn_dim=GOOD[1], hidden_dim=GOOD[2]).to(dev()).eval()

    def run_good():
        out = good.forward_bags(feats.to(dev()), offsets, want_pooled=True)
        torch.cuda.synchronize()
        return [cpu(t) for t in out]

    before = run_good()
    # (1024, ...) under attention pooling: the score kernel's LDS limit, 16 F 4 + 16 (threads / 64) 4 <= 64 KiB, ends at F = 1020
    for dims, poolings in [(d, ("attention", "mean")) for d in REFUSED] + [((1024, 31, 17, 2), ("attention",))]:
        for pooling in poolings:
            if pooling == "mean" and dims[1] > 256:
                continue
            x, offs, _ = _small_batch(dims[0], dims[3])
            m = mil.MILClassifier(dims[0], dims[3], pooling, attn_dim=dims[1], hidden_dim=dims[2]).to(dev()).eval()
            for _ in range(2):  # the refused object refuses again, it does not fall over
                with pytest.raises(capi.HipacError):
                    m.forward_bags(x.to(dev()), offs, want_pooled=True)
            after = run_good()
            assert all(torch.equal(p, q) for p, q in zip(before, after)), (dims, pooling)
    # and F = 1024 is inside the limits of the poolings that have no score kernel
    m = mil.MILClassifier(1024, 2, "max", attn_dim=31, hidden_dim=17).to(dev()).eval()
    x, offs, _ = _small_batch(1024, 2)
    logits, _, pooled = m.forward_bags(x.to(dev()), offs, want_pooled=True)
    assert torch.equal(cpu(pooled), torch.stack([x[:3].max(dim=0).values, x[3:].max(dim=0).values]))
