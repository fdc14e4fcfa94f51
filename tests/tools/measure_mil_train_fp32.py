"""How far torch's own float32 autograd lands from its float64 autograd on exactly the inputs of
tests/test_gpu_mil_train.py (CPU only).  Writes tests/golden/mil_train_fp32_distances.json:

    {"cases": {case id: {tensor: max|f32 - f64| / max|f64|, "attn_U_bias_abs": max|f32 db_U|}},
     "per_group": {"F,A,hidden,C,pooling": {tensor: the largest distance over that group's cases, ...}},
     "adam": {pooling: {tensor: |p32 - p64|_2 / |p64 - p0|_2 after five Adam steps}}}

The GPU test gates the native step at 10 x the per-group figure of each tensor (the factor tests/test_gpu_train.py
leaves between its measured 5e-5 and its 5e-4 gate).  A group is the cases that run the SAME computation -- the same
dims and the same pooling -- on different data (class weights or not, identity or permuted rows, and the two-batch
accumulate case); nothing is pooled across poolings or dims.  Inside a group the largest figure is taken because a
single case's figure is one draw of rounding noise: torch's float32 lands within 6e-9 of float64 on classifier.2.bias
in one case, a tenth of the format's half-ulp 2^-24 = 6e-8, which no float32 computation can be asked to repeat.
aggregator.attn_U.bias has gradient 0 in exact arithmetic and takes the absolute figure instead.

    python tests/tools/measure_mil_train_fp32.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mil_train_cases as cases  # noqa: E402

UB = "aggregator.attn_U.bias"


def distances(r32, r64):
    (l32, z32, g32), (l64, z64, g64) = r32, r64
    d = {k: cases.rel(g32[k], g64[k]) for k in g64 if k != UB}
    d["logits"] = cases.rel(z32, z64)
    d["loss_rel"] = abs(float(l32) - float(l64)) / abs(float(l64))
    if UB in g32:
        d["attn_U_bias_abs"] = float(g32[UB].abs().max())
        d["attn_U_bias_abs_f64"] = float(g64[UB].abs().max())
    return d


def main():
    out = {"cases": {}, "per_group": {}, "adam": {}}

    def record(cid, dims, pooling, d):
        out["cases"][cid] = d
        agg = out["per_group"].setdefault(",".join(map(str, dims)) + "," + pooling, {})
        for k, v in d.items():
            agg[k] = max(agg.get(k, 0.0), v)
        print(cid, {k: f"{v:.2e}" for k, v in d.items()}, flush=True)

    for cid, dims, pooling, weighted, permuted in cases.case_list():
        model = cases.make_model(dims, pooling)
        feats, rows, offsets, labels, cw = cases.make_inputs(dims, permuted)
        cw = cw if weighted else None
        r = [cases.autograd_reference(model, pooling, feats, rows, offsets, labels, cw, dt) for dt in (torch.float32, torch.float64)]
        record(cid, dims, pooling, distances(*r))
    for pooling in cases.POOLINGS:  # the accumulate test: the gradients of two batches added, logits / loss of the second
        dims = cases.DIMS[0]
        model = cases.make_model(dims, pooling)
        a, b = cases.accumulate_inputs(dims)
        r = []
        for dt in (torch.float32, torch.float64):
            ra, rb = cases.autograd_reference(model, pooling, *a, dt), cases.autograd_reference(model, pooling, *b, dt)
            r.append((rb[0], rb[1], {k: ra[2][k] + rb[2][k] for k in ra[2]}))
        record(f"accumulate-{pooling}", dims, pooling, distances(*r))
    for pooling in cases.POOLINGS:  # five Adam steps: error of the movement, float32 twin against float64 twin
        model = cases.make_model(cases.DIMS[0], pooling)
        p64 = cases.adam_twin(model, pooling, torch.float64)
        p32 = cases.adam_twin(model, pooling, torch.float32)
        p0 = model.state_dict()
        out["adam"][pooling] = {k: float((p32[k].double() - p64[k]).norm() / (p64[k] - p0[k].double()).norm()) for k in p64}
        print("adam", pooling, {k: f"{v:.2e}" for k, v in out["adam"][pooling].items()}, flush=True)
    path = os.path.join(os.path.dirname(HERE), "golden", "mil_train_fp32_distances.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
