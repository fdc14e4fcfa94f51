"""How far torch's own float32 CPU computation lands from the float64 references on exactly the inputs of
tests/test_gpu_mil_edge.py (tests/mil_edge_cases.py): float32 autograd over mil.MILClassifier for the training step, the
float32 evaluation of the restatement for the inference head.  CPU only, one thread; never touches the native code.
Writes tests/golden/mil_edge_fp32_distances.json:

    {"factor": 10.0, "how": this command,
     "cases": {case id: {figure: value}},
     "per_group": {"train|infer:F,A,hidden,C,pooling,kind": {figure: the largest value over that group's cases}}}

Figures: a tensor's name (logits, attn, pooled, a state_dict key) is max|f32 - f64| / max|f64|; "row:" + a 2-d gradient's key
is the row-wise metric of tests/mil_edge_cases.py (plain kind only); attn_U_bias_abs is max|f32 db_U| (exact value 0);
loss_abs is |loss32 - loss64| (recorded, not a gate: the loss is gated at 1e-5 relative + 1e-6).  The GPU test gates the
native code at 10 x the per-group figure.  tests/test_oracle_mil_edge.py checks that this file reproduces the committed
json and that no gate exceeds 1e-3.

    python tests/tools/measure_mil_edge_fp32.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mil_edge_cases as cases  # noqa: E402


def main():
    out = cases.measure(log=lambda s: print(s, flush=True))
    with open(cases.JSON_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("per group:")
    for g, figs in sorted(out["per_group"].items()):
        print(f"  {g}: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(figs.items())))
    worst = max(v for figs in out["per_group"].values() for k, v in figs.items() if k not in cases.UNCAPPED)
    print(f"largest rel / row_rel figure {worst:.3e} (x {cases.FACTOR:g} must stay under {cases.CAP:g})")
    print("wrote", cases.JSON_PATH)


if __name__ == "__main__":
    main()
