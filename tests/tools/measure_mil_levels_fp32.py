"""How far torch's own float32 autograd lands from its float64 autograd on exactly the inputs of
tests/test_gpu_mil_levels.py (CPU only).  Writes tests/golden/mil_levels_fp32_distances.json:

    {"cases": {case id: {tensor: max|f32 - f64| / max|f64|, "attn_U_bias_abs": max|f32 db_U|}},
     "per_group": {"F,A,hidden,C,L": {tensor: the largest distance over that group's cases, ...}},
     "eval": {"F,A,hidden,C,L": {"logits" | "attn" | "pooled": distance of the forward without gradients}}}

The GPU test gates the native step and the native forward at 10 x the per-group figure of each tensor (the rule and the
factor of tests/test_gpu_mil_train.py, tests/test_gpu_mil_heads.py and tests/test_gpu_mil_gated.py).  A group is the cases
that run the SAME computation -- the same (F, A, hidden, C, L) -- on different data (class weights or not, identity or
permuted rows, the two-batch accumulate case, the batch with a row of no level); nothing is pooled across dims.
aggregator.attn_U.bias (L values) has gradient 0 in exact arithmetic and takes the absolute figure.

    python tests/tools/measure_mil_levels_fp32.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mil_levels_cases as cases  # noqa: E402

UB = "aggregator.attn_U.bias"


def distances(r32, r64):
    (l32, z32, a32, g32), (l64, z64, a64, g64) = r32, r64
    d = {k: cases.rel(g32[k], g64[k]) for k in g64 if k != UB}
    d["logits"] = cases.rel(z32, z64)
    d["loss_rel"] = abs(float(l32) - float(l64)) / abs(float(l64))
    if a32 is not None:
        d["attn"] = cases.rel(a32, a64)
    d["attn_U_bias_abs"] = float(g32[UB].abs().max())
    d["attn_U_bias_abs_f64"] = float(g64[UB].abs().max())
    return d


def main():
    out = {"cases": {}, "per_group": {}, "eval": {}}

    def record(cid, dims, d):
        out["cases"][cid] = d
        agg = out["per_group"].setdefault(cases.group_key(dims), {})
        for k, v in d.items():
            agg[k] = max(agg.get(k, 0.0), v)
        print(cid, {k: f"{v:.2e}" for k, v in d.items()}, flush=True)

    for cid, dims, weighted, permuted in cases.case_list():
        twin = cases.make_twin(dims)
        feats, rows, offsets, labels, cw, lv = cases.make_inputs(dims, permuted)
        cw = cw if weighted else None
        record(cid, dims, distances(*[cases.reference(twin, feats, rows, offsets, labels, cw, lv, dt) for dt in (torch.float32, torch.float64)]))
    dims = cases.ACC_DIMS  # the accumulate test: the gradients of two batches added; logits, loss of the second
    twin = cases.make_twin(dims)
    a, b = cases.accumulate_inputs(dims)
    r = []
    for dt in (torch.float32, torch.float64):
        ra, rb = cases.reference(twin, *a, dt), cases.reference(twin, *b, dt)
        r.append((rb[0], rb[1], None, {k: ra[3][k] + rb[3][k] for k in ra[3]}))
    record("accumulate", dims, distances(*r))
    dims = cases.DIMS[0]  # the batch with a row of no level
    twin = cases.make_twin(dims)
    feats, rows, offsets, labels, cw, lv = cases.make_inputs(dims, True)
    lv = lv.clone()
    lv[cases.NOISE_ROW] = 200
    record("no-level-row", dims, distances(*[cases.reference(twin, feats, rows, offsets, labels, cw, lv, dt) for dt in (torch.float32, torch.float64)]))
    for dims in cases.DIMS:  # the forward without gradients (hipac_mil_levels_forward): identity rows
        twin = cases.make_twin(dims)
        feats, _, offsets, _, _, lv = cases.make_inputs(dims, False)
        e32, e64 = (cases.eval_reference(twin, feats, offsets, lv, dt) for dt in (torch.float32, torch.float64))
        d = {name: cases.rel(x, y) for name, x, y in zip(("logits", "attn", "pooled"), e32, e64)}
        out["eval"][cases.group_key(dims)] = d
        print("eval", dims, {k: f"{v:.2e}" for k, v in d.items()}, flush=True)
    path = os.path.join(os.path.dirname(HERE), "golden", "mil_levels_fp32_distances.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
