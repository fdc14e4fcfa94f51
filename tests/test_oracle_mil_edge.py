"""CPU: the cases, references and gates that tests/test_gpu_mil_edge.py holds the single-head MIL head to
(tests/mil_edge_cases.py, tests/mil_edge_cpu.py, tests/golden/mil_edge_fp32_distances.json).

  * the committed json is what tests/tools/measure_mil_edge_fp32.py reproduces;
  * the conditions on the gates hold: no rel / row_rel gate above 1e-3, every gated tensor's float64 reference is non-zero,
    every peaked case has a bag whose largest score exceeds 89 (expf without the max shift overflows there), the bag sizes
    sit on the tile edges they were chosen for;
  * the stand-in's formulas in float64 land on the float64 autograd references, so its manual backward is the step's;
  * the float32 stand-in without a fault passes every gate, the two degenerate cases' exact zeros included;
  * the stand-in with each fault of mil_edge_cpu.FAULTS fails on at least one case, the cases built for that fault among
    them -- the test prints which.  A fault that no case catches means the cases or the metrics are too weak.
"""
import math

import numpy as np
import pytest
import torch

import mil_edge_cases as cases
import mil_edge_cpu as cpu

QUIET = lambda s: None


@pytest.fixture(scope="module")
def measured():
    return cases.measure()


def run(impl, case):
    """What the GPU test obtains from the native code, from the stand-in."""
    s = cases.setup(case)
    sd = s[0].state_dict()
    if case.what == "infer":
        return impl.infer(sd, case.pooling, s[1], s[2])
    if case.what == "acc":
        first = impl.step(sd, case.pooling, *s[1])
        return impl.step(sd, case.pooling, *s[2], prev=first[2])
    return impl.step(sd, case.pooling, *s[1])


# ---------------------------------------------------------------------------------------------
# the json and the conditions on it
# ---------------------------------------------------------------------------------------------
def test_recorded_distances_are_what_the_tool_reproduces(measured):
    rec = cases.recorded()
    assert rec["factor"] == cases.FACTOR == 10.0 and rec["how"] == cases.HOW
    assert rec["cases"] == measured["cases"]
    assert rec["per_group"] == measured["per_group"]
    ids = [c.id for c in cases.all_cases()]
    assert sorted(rec["cases"]) == sorted(ids) and len(set(ids)) == len(ids)
    assert sorted(rec["per_group"]) == sorted({cases.group_of(c) for c in cases.all_cases()})  # no case left out of its group


def test_no_gate_exceeds_the_cap(measured):
    worst = ("", "", 0.0)
    for g, figs in measured["per_group"].items():
        for k, v in figs.items():
            assert math.isfinite(v), (g, k)
            if k not in cases.UNCAPPED:
                assert cases.FACTOR * v <= cases.CAP, (g, k, v)
                worst = max(worst, (g, k, v), key=lambda t: t[2])
    print(f"[mil_edge] largest rel / row_rel figure: {worst[2]:.3e} ({worst[0]} {worst[1]}), gate {cases.FACTOR * worst[2]:.3e} <= {cases.CAP:g}")
    # the absolute gate of db_U stays far under every gradient it sits next to
    assert max(figs.get("attn_U_bias_abs", 0.0) for figs in measured["per_group"].values()) * cases.FACTOR < 1e-6


def test_every_gated_reference_is_non_zero():
    for case in cases.all_cases():
        ref = cases.reference(case)
        if case.what == "infer":
            tensors = {"logits": ref[0], "pooled": ref[2], **({"attn": ref[1]} if case.pooling == "attention" else {})}
        else:
            tensors = {"logits": ref[1], **({"attn": ref[3]} if case.pooling == "attention" else {})}
            assert math.isfinite(float(ref[0]))
            for k, g in ref[2].items():
                if case.special == "c1":  # one class: loss and gradients are exactly 0 in float64 too
                    assert float(ref[0]) == 0.0 and float(g.abs().max()) == 0.0, (case.id, k)
                elif k == cases.UB or (case.special == "one" and k in cases.ATTENTION_GRADS):
                    assert float(g.abs().max()) < 1e-15, (case.id, k)  # 0 in exact arithmetic
                else:
                    tensors[k] = g
        for k, t in tensors.items():
            assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0.0, (case.id, k)


def test_peaked_scores_overflow_expf_without_the_max_shift():
    peaked = [c for c in cases.all_cases() if c.kind == "peaked"]
    assert len(peaked) >= 40
    for case in peaked:
        s, offsets = cases.scores64(case)
        tops = [float(s[a:b].max()) for a, b in zip(offsets[:-1], offsets[1:])]
        spread = max(float(s[a:b].max() - s[a:b].min()) for a, b in zip(offsets[:-1], offsets[1:]))
        assert max(tops) > 89.0, (case.id, max(tops))  # expf(88.73) is float32's largest finite value
        print(f"[mil_edge] {case.id}: largest score {max(tops):.1f}, largest range inside a bag {spread:.1f}")


def test_bag_sizes_sit_on_the_edges_they_were_chosen_for():
    S = cases.SIZES
    ends = np.cumsum(S["tile"])
    assert list(ends[:2]) == [64, 128] and ends[3] == 192 and ends[4] == 320 and S["tile"][2] == 1 and S["tile"][5] == 1
    assert (ends[1] % 64, (ends[2] - 1) % 64, (ends[5] - 1) % 64) == (0, 0, 0)  # single-row bags at a tile's start; two whole tiles
    assert len(S["many"]) == 257 and sum(S["many"]) == 314 and max(S["many"][:64]) == 1  # 64 segments in the first tile
    assert 130 in S["mix"] and sum(S["pair"]) == 4 and S["one"] == [1]
    assert sum(S["big"]) == 2105 and (S["big"][0] + 63) // 64 == 33
    assert {c.sizes for c in cases.train_cases() if c.dims[0] == 2048} >= {"big"}
    assert not [c for c in cases.train_cases() if c.sizes == "big" and c.dims[0] != 2048]
    assert sum(1 for c in cases.train_cases() if not c.permuted) == 3  # the identity row index once per pooling
    assert all(c.dims[0] <= 1020 for c in cases.infer_cases() if c.pooling == "attention")


# ---------------------------------------------------------------------------------------------
# the stand-in: in float64 the reference, in float32 inside every gate
# ---------------------------------------------------------------------------------------------
def test_the_standin_in_float64_is_the_reference():
    impl = cpu.StandIn(dtype=torch.float64)
    for case in cases.all_cases():
        got = run(impl, case)
        for k, v in cases.figures(case, got).items():
            bound = 1e-15 if k in cases.UNCAPPED else 1e-11
            assert v <= bound, (case.id, k, v)
        if case.what != "infer" and case.special == "one":  # the excluded attention gradients: the same zeros as autograd's
            assert all(float(got[2][k].abs().max()) < 1e-15 for k in cases.ATTENTION_GRADS), case.id


def test_standin_passes_every_gate():
    impl = cpu.StandIn()
    lines = []
    for case in cases.all_cases():
        bad = cases.failures(case, run(impl, case), log=lines.append)
        assert bad == [], (case.id, bad)
    for case in cases.train_cases():
        if case.special:
            print("\n".join(l for l in lines if f" {case.id}: " in l))


# ---------------------------------------------------------------------------------------------
# one injected fault at a time: some case must notice -- and the cases built for that boundary among them
# ---------------------------------------------------------------------------------------------
TARGETS = {
    "last_attn_unit": ["train-attention-F36A33h5C3-mix-plain", "train-attention-F68A65h255C16-tile-plain",
                       "infer-attention-F36A33h5C3-mix-plain", "infer-attention-F68A65h255C16-tile-plain"],
    "feature_tail": ["train-attention-F68A65h255C16-mix-plain", "train-attention-F100A250h256C2-mix-plain"],
    "tile_last_row": ["train-attention-F36A33h5C3-tile-plain", "train-mean-F4A1h3C2-tile-plain", "train-max-F2048A31h17C2-tile-plain",
                      "infer-attention-F68A65h255C16-tile-plain"],
    "bag_edge": ["train-attention-F68A65h255C16-tile-plain", "train-attention-F4A1h3C2-many-plain", "train-mean-F36A33h5C3-tile-plain",
                 "train-max-F100A250h256C2-many-plain", "infer-attention-F1020A31h17C2-many-plain"],
    "mean_by_segment": ["train-mean-F36A33h5C3-mix-plain", "infer-mean-F2048A31h17C2-mix-plain"],
    "max_from_zero": ["train-max-F36A33h5C3-many-plain", "train-max-F4A1h3C2-one-plain", "infer-max-F68A65h255C16-one-plain"],
    "no_max_shift": ["train-attention-F36A33h5C3-mix-peaked", "train-attention-F36A33h5C3-pair-peaked",
                     "train-attention-F2048A31h17C2-big-peaked", "infer-attention-F1020A31h17C2-mix-peaked"],
    "accumulate_overwrites": [cases.ACC_CASE.id],
    "score_group_clamp": ["infer-attention-F36A33h5C3-mix-plain", "infer-attention-F4A1h3C2-pair-plain"],  # n = 330, n = 4
}


@pytest.mark.parametrize("fault", cpu.FAULTS)
def test_fault_is_caught(fault):
    impl = cpu.StandIn(fault)
    caught, total = {}, 0
    for case in cases.all_cases():
        total += 1
        bad = cases.failures(case, run(impl, case), log=QUIET)
        if bad:
            caught[case.id] = bad[0]
    assert caught, f"no case notices the fault {fault}"
    print(f"[mil_edge] fault {fault}: caught by {len(caught)} of {total} cases: " + "; ".join(list(caught)[:6])
          + (" ..." if len(caught) > 6 else ""))
    for t in TARGETS[fault]:
        assert t in caught, f"the case built for it, {t}, does not notice the fault {fault}"
        k, v, g = caught[t]
        fmt = lambda x: format(x, ".3g") if isinstance(x, float) else str(x)
        print(f"[mil_edge]     {t}: {k} {fmt(v)} over its gate {fmt(g)}")
    assert sorted(TARGETS) == sorted(cpu.FAULTS)
