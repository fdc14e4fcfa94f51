"""How far the float32 stand-ins of the training head's primitives (tests/head_cpu.py: plain torch float32 ops) land
from their float64 references on exactly the inputs of tests/test_gpu_head.py (tests/head_cases.py).  CPU only; never
touches the native code.  Writes tests/golden/head_fp32_distances.json:

    {"factor": 10.0, "how": this command,
     "cases": {case id: {"primitive.tensor.input kind": max|f32 - f64| / max|f64|}},
     "per_group": {"primitive.tensor.input kind": the largest figure over that group's cases}}

The GPU test gates the cross-entropy, Adam and NT-Xent outputs at 10 x the per-group figure (the rule of
tests/test_gpu_mil_train.py).  A group is one primitive, one tensor and one input kind; nothing is pooled across
primitives.  Adam's p is measured on the move p_new - p_old.  The linear layers are not in here: their gate is derived
(tests/head_cases.py).  tests/test_oracle_head.py checks that this file reproduces the committed json.

    python tests/tools/measure_head_fp32.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import head_cases as cases  # noqa: E402


def main():
    out = cases.measure(log=lambda s: print(s, flush=True))
    with open(cases.JSON_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("per group:")
    for k, v in sorted(out["per_group"].items()):
        print(f"  {k} {v:.3e}")
    print("wrote", cases.JSON_PATH)


if __name__ == "__main__":
    main()
