"""CPU: the references, cases and gates that tests/test_gpu_head.py holds the training head's kernels to
(tests/head_cpu.py, tests/head_cases.py, tests/golden/head_fp32_distances.json).

  * the float64 references agree with torch autograd / torch.optim.Adam in float64 on the cases;
  * the float32 stand-in without a fault passes every bound and gate, and the committed json is what
    tests/tools/measure_head_fp32.py reproduces;
  * the stand-in with each fault of head_cpu.FAULTS fails on at least one case -- the test prints which.  A fault that
    no case catches means the cases or the metric are too weak.
"""
import math

import numpy as np
import pytest
import torch

import head_cases as cases
import head_cpu as H


@pytest.fixture(scope="module")
def measured():
    return cases.measure()


# ---------------------------------------------------------------------------------------------
# the float64 references against torch in float64
# ---------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-12):
    return cases.rel(a, b) <= tol


@pytest.mark.parametrize("shape", cases.LINEAR_SHAPES, ids=str)
def test_linear_reference_is_float64_autograd(shape):
    d = cases.linear_inputs(shape)
    for relu in (False, True):
        x, w, b = (torch.from_numpy(H.f64(d[k])).requires_grad_(True) for k in ("x", "w", "b"))
        y = torch.nn.functional.linear(x, w, b)
        y = torch.relu(y) if relu else y
        y.backward(torch.from_numpy(H.f64(d["dy"])))
        assert _close(H.linear_forward(d["x"], d["w"], d["b"], relu), y.detach().numpy())
        # the reference takes the mask from a given y: float64 y here, the same units as autograd's
        dx, dw, db, dym = H.linear_backward(d["x"], d["w"], d["dy"], y.detach().numpy() if relu else None, d["dw0"], d["db0"])
        assert _close(dx, x.grad.numpy()) and _close(dw, w.grad.numpy() + H.f64(d["dw0"])) and _close(db, b.grad.numpy() + H.f64(d["db0"]))
        # the float32 y the cases hand to the backward switches the same units (rounding keeps the sign)
        if relu:
            assert ((d["y"] > 0) == (y.detach().numpy() > 0)).all()
            assert (dym == np.where(d["y"] > 0, H.f64(d["dy"]), 0.0)).all()


def test_special_mask_places():
    y, d = cases.mask_special_y(), cases.linear_inputs(cases.MASK_SHAPE)
    assert not np.any((np.abs(y) > 0) & (np.abs(y) < cases.FLT_MIN))  # no denormals: their compare depends on the mode
    dym = H.linear_backward(d["x"], d["w"], d["dy"], y)[3].astype(np.float32)
    for (r, c), (val, kept) in cases.MASK_PLACES.items():
        assert cases.same_bits(y[r, c], val) and d["dy"][r, c] != 0
        assert cases.same_bits(dym[r, c], d["dy"][r, c] if kept else np.float32(0.0)), (r, c)
    assert sorted(k for k, v in cases.MASK_PLACES.items() if v[1]) == [(7, 5)]


@pytest.mark.parametrize("case", cases.ce_case_list(), ids=lambda c: c[0])
def test_cross_entropy_reference_is_float64_autograd(case):
    logits, labels, cw = cases.ce_inputs(*case[1:])
    l = torch.from_numpy(H.f64(logits)).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(l, torch.from_numpy(labels), weight=None if cw is None else torch.from_numpy(H.f64(cw)))
    loss.backward()
    rl, rd = H.cross_entropy(logits, labels, cw)
    assert _close(rl, float(loss.detach())) and _close(rd, l.grad.numpy())
    if case[2] == "zero":
        assert cw[labels[0]] == 0 and (labels == labels[0]).sum() >= 1


def test_bad_label_rows_count_as_weight_zero():
    """What the bad-label test of the kernel compares the good rows with -- the batch without the three rows -- is what
    torch computes when those rows are ignored."""
    logits, labels, cw, good = cases.ce_bad_label_inputs()
    assert sorted(cases.BAD_LABELS) == [0, 128, 256] and [labels[r] for r in (0, 128, 256)] == [-1, logits.shape[1], 2 ** 40]
    lab = labels.copy()
    lab[list(cases.BAD_LABELS)] = -100
    l = torch.from_numpy(H.f64(logits)).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(l, torch.from_numpy(lab), weight=torch.from_numpy(H.f64(cw)), ignore_index=-100)
    loss.backward()
    rl, rd = H.cross_entropy(logits[good], labels[good], cw)
    assert _close(rl, float(loss.detach())) and _close(rd, l.grad.numpy()[good])


@pytest.mark.parametrize("case", [c for c in cases.adam_case_list() if c[1] <= 257], ids=lambda c: c[0])
def test_adam_reference_is_torch_adam_in_float64(case):
    _, n, kind, mode = case
    p, grads, m, v, step, b1, b2, eps = cases.adam_inputs(n, kind, mode)
    q = torch.from_numpy(H.f64(p)).requires_grad_(True)
    opt = torch.optim.Adam([q], lr=H.f32s(cases.ADAM_LR), betas=(H.f32s(b1), H.f32s(b2)), eps=H.f32s(eps))
    if step > 1:  # a start from non-zero state at a large step
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(H.f64(m)),
                        "exp_avg_sq": torch.from_numpy(H.f64(v))}
    for g in grads:
        q.grad = torch.from_numpy(H.f64(g))
        opt.step()
    rp, rm, rv = H.adam_steps(p, grads, m, v, step, cases.ADAM_LR, b1, b2, eps)
    assert cases.rel(rp - H.f64(p), q.detach().numpy() - H.f64(p)) <= 1e-9  # torch's own float64 rounding of p
    assert _close(rm, opt.state[q]["exp_avg"].numpy()) and _close(rv, opt.state[q]["exp_avg_sq"].numpy())
    if kind == "zeros":
        assert all((g[cases.adam_zero_places(n)] == 0).all() for g in grads)
    if kind == "small_p":
        assert np.abs(p).max() <= 1e-3


def test_the_closed_forms_in_float64_are_the_references():
    """The stand-in's formulas, evaluated in float64, land on the references: what separates the float32 stand-in from
    them is float32 alone.  For NT-Xent this holds the closed form of csrc/ntxent.hip's header to the reference's autograd."""
    impl = H.StandIn(dtype=torch.float64)
    for shape in cases.LINEAR_SHAPES:
        worst = max(cases.linear_ratios(impl, shape).values())
        assert worst <= 1e-6, (shape, worst)
    for prim, (case_list, figures) in cases.FIGURES.items():
        for case in case_list():
            for k, v in figures(impl, case).items():
                # the zero row's own gradient is the one place where autograd and the closed form round apart: 1e12 x 1e-16
                assert v <= (1e-9 if prim == "adam" and ".move." in k else 1e-11), (case[0], k, v)


def test_zero_row_gradient_is_large_and_finite():
    shape = cases.NTX_VARIANT_SHAPES[0]
    _, dz = cases.ntxent_reference(shape, "zero_row")
    row = np.abs(dz[cases.NTX_ZERO_ROW]).max()
    assert np.isfinite(dz).all() and 1e9 < row < 1e13 and np.abs(np.delete(dz, cases.NTX_ZERO_ROW, 0)).max() < 10


# ---------------------------------------------------------------------------------------------
# the stand-in without a fault: inside every bound and gate; the json is reproducible
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.LINEAR_SHAPES, ids=str)
def test_standin_is_inside_the_linear_bound(shape):
    r = cases.linear_ratios(H.StandIn(), shape)
    k = max(r, key=r.get)
    print(f"[head] linear {shape}: worst bound ratio {r[k]:.3f} ({k})")
    assert all(v <= 1.0 for v in r.values()), {k: v for k, v in r.items() if not v <= 1.0}


def test_recorded_distances_are_what_the_tool_reproduces(measured):
    rec = cases.recorded()
    assert rec["factor"] == cases.FACTOR == 10.0 and rec["how"] == cases.HOW
    assert rec["cases"] == measured["cases"]
    assert rec["per_group"] == measured["per_group"]
    ids = [c[0] for case_list, _ in cases.FIGURES.values() for c in case_list()]
    assert sorted(rec["cases"]) == sorted(ids) and len(set(ids)) == len(ids)


def test_standin_passes_every_gate(measured):
    for cid, figs in measured["cases"].items():
        assert cases.over_gate(cid, figs, log=lambda s: None) == []
    for k, v in measured["per_group"].items():
        assert math.isfinite(v), k
        print(f"[head] gate {k}: {cases.FACTOR:g} x {v:.3e}")


# ---------------------------------------------------------------------------------------------
# one injected fault at a time: some case must notice -- and the case that was built for that boundary among them
# ---------------------------------------------------------------------------------------------
TARGETS = {
    "k_tail": [(64, 64, 33), (129, 1, 95), (15, 17, 70)],  # K = 33 forward; N = 1, M = 129 and K = 95 as reduction lengths
    "mask_ge": [(16, 128, 512), (15, 17, 70)],
    "acc_overwrite": [(63, 65, 32), (16, 128, 512)],
    "db_rows16": [(129, 1, 95), (15, 17, 70)],
    "mean_over_m": ["ce-513x5-w_random-randn", "ce-256x2-w_zero-randn"],
    "group_tail": ["ce-257x64-w_none-randn", "ce-513x5-w_random-spread1e4"],
    "no_max_shift": ["ce-513x5-w_none-spread1e4"],
    "no_stride": [f"adam-n{H.ADAM_GRID_ELEMS + 1}-randn-A-default", f"adam-n{H.ADAM_GRID_ELEMS + 1}-x1e-12-B-t1000"],
    "eps_in_sqrt": ["adam-n257-small_p-A-default", "adam-n255-x1e-12-A-betas"],
    "bc_prev_step": ["adam-n257-randn-A-default", "adam-n255-zeros-A-betas"],
    "diag_in_lse": ["ntxent-n128-d32-t0.1-plain", "ntxent-n3-d65-t0.05-identical"],
    "pair_no_wrap": ["ntxent-n129-d32-t0.1-plain", "ntxent-n2-d63-t0.07-plain"],
    "lse_tail": ["ntxent-n129-d32-t0.1-plain", "ntxent-n129-d32-t0.1-zero_row"],
    "no_projection": ["ntxent-n128-d32-t0.1-plain", "ntxent-n37-d300-t0.07-plain"],
}


def _report(prim, fault, caught, total):
    assert caught, f"no {prim} case notices the fault {fault}"
    print(f"[head] {prim} fault {fault}: caught by {len(caught)} of {total} cases: "
          + "; ".join(f"{c} ({k} {v:.3g})" for c, (k, v) in list(caught.items())[:4]) + (" ..." if len(caught) > 4 else ""))
    for t in TARGETS[fault]:
        assert t in caught, f"the case built for it, {t}, does not notice the fault {fault}"
        print(f"[head]     {t}: {caught[t][0]} {caught[t][1]:.3g}")


@pytest.mark.parametrize("fault", H.FAULTS["linear"])
def test_linear_fault_is_caught(fault):
    impl = H.StandIn(fault)
    caught = {}
    for shape in cases.LINEAR_SHAPES:
        bad = {k: v for k, v in cases.linear_ratios(impl, shape).items() if not v <= 1.0}
        if bad:
            k = max(bad, key=bad.get)
            caught[shape] = (k, bad[k])
    _report("linear", fault, caught, len(cases.LINEAR_SHAPES))


@pytest.mark.parametrize("prim,fault", [(p, f) for p in ("ce", "adam", "ntxent") for f in H.FAULTS[p]])
def test_fault_is_caught(prim, fault):
    impl = H.StandIn(fault)
    case_list, figures = cases.FIGURES[prim]
    caught = {}
    for case in case_list():
        bad = cases.over_gate(case[0], figures(impl, case), log=lambda s: None)
        if bad:
            caught[case[0]] = (f"{bad[0][0]} over its gate {bad[0][2]:.3g}:", bad[0][1])
    _report(prim, fault, caught, len(case_list()))
