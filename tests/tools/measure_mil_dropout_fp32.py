"""How far torch's own float32 autograd lands from its float64 autograd on exactly the inputs of
tests/test_gpu_mil_dropout.py, with the same explicit dropout masks on both sides (CPU only).  Writes
tests/golden/mil_dropout_fp32_distances.json:

    {"cases": {case id: {tensor: max|f32 - f64| / max|f64|, "attn_U_bias_abs": max|f32 db_U|, "mc_logits": ..., "mc_attn": ...}},
     "per_group": {"F,A,hidden,C,pooling": {tensor: the largest distance over that group's cases, ...}}}

The rule is tests/tools/measure_mil_train_fp32.py's: the GPU test gates each tensor at 10 x the per-group figure, a group
being the cases that run the same computation (same dims, same pooling) on different data -- here the two dropout
probabilities, training steps 0 and 1, and the seven Monte-Carlo samples.  "mc_logits" is the per-sample logits of the
Monte-Carlo forward (T = 7, all samples in one figure), "mc_attn" its per-sample attention weights.

    python tests/tools/measure_mil_dropout_fp32.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mil_dropout_cpu as cpu  # noqa: E402

UB = "aggregator.attn_U.bias"


def main():
    out = {"cases": {}, "per_group": {}}
    for cid, dims, pooling, p in cpu.case_list():
        model = cpu.make_model(dims, pooling)
        feats, rows, offsets, labels, cw = cpu.make_inputs(dims, True)
        d = {}
        for step in (0, 1):
            (l32, z32, g32), (l64, z64, g64) = [cpu.train_reference(model, pooling, feats, rows, offsets, labels, cw, p, cpu.SEED, step, dt)
                                                for dt in (torch.float32, torch.float64)]
            cur = {k: cpu.rel(g32[k], g64[k]) for k in g64 if k != UB}
            cur["logits"] = cpu.rel(z32, z64)
            cur["loss_rel"] = abs(float(l32) - float(l64)) / abs(float(l64))
            if UB in g32:
                cur["attn_U_bias_abs"] = float(g32[UB].abs().max())
            for k, v in cur.items():
                d[k] = max(d.get(k, 0.0), v)
        x = cpu.make_inputs(dims, False)[0]
        (z32, w32), (z64, w64) = [cpu.mc_reference(model, pooling, x, offsets, p, cpu.SEED, 0, max(cpu.TS), dt)
                                  for dt in (torch.float32, torch.float64)]
        d["mc_logits"] = cpu.rel(z32, z64)
        if w64 is not None:
            d["mc_attn"] = cpu.rel(w32, w64)
        out["cases"][cid] = d
        agg = out["per_group"].setdefault(cpu.group_key(dims, pooling), {})
        for k, v in d.items():
            agg[k] = max(agg.get(k, 0.0), v)
        print(cid, {k: f"{v:.2e}" for k, v in d.items()}, flush=True)
    path = os.path.join(os.path.dirname(HERE), "golden", "mil_dropout_fp32_distances.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
