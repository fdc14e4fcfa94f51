"""How far numpy's own float32 arithmetic lands from float64 on the inputs of tests/test_gpu_knn.py: the figures behind that
test's gates (10 x, the rule of tests/test_gpu_mil_train.py).  CPU only; never sees the code under test.

    python tests/tools/measure_knn_fp32.py      -> tests/golden/knn_fp32_distances.json

Per group (the cases of one F): ``sim`` = the largest |float32 - float64| over ALL pair similarities of the group's cases
(cosine: float32 dot products through numpy's float32 matmul, scaled by float32 inverse norms, against the same in float64);
``inv_norms`` = the largest relative error of the float32 inverse norms.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import knn_cases as cases  # noqa: E402
import knn_cpu as cpu  # noqa: E402


def measure(shape):
    x, q_rows, b_rows = cases.float64_inputs(*shape)
    q64, b64 = cpu.inv_norms(x, q_rows), cpu.inv_norms(x, b_rows)
    q32, b32 = cpu.inv_norms(x, q_rows, np.float32), cpu.inv_norms(x, b_rows, np.float32)
    s64 = cpu.similarities(x, q_rows, b_rows, q64, b64)
    s32 = cpu.similarities(x, q_rows, b_rows, q32, b32, np.float32)
    assert s32.dtype == np.float32
    sim = float(np.abs(s32.astype(np.float64) - s64).max())
    inv = float(max(np.abs(q32 / q64 - 1).max(), np.abs(b32 / b64 - 1).max()))
    return sim, inv


def main():
    per_group, per_case = {}, {}
    for shape in cases.FLOAT64_SHAPES + cases.SPLIT_SHAPES:
        sim, inv = measure(shape)
        per_case[cases.shape_id(shape)] = {"sim": sim, "inv_norms": inv}
        g = per_group.setdefault(cases.group_key(shape[0]), {"sim": 0.0, "inv_norms": 0.0})
        g["sim"], g["inv_norms"] = max(g["sim"], sim), max(g["inv_norms"], inv)
        print(f"{cases.shape_id(shape):>20}: sim {sim:.2e}, inv_norms {inv:.2e}")
    doc = {"factor": 10.0, "metric": "sim: max |a - b|; inv_norms: max |a / b - 1|", "per_group": per_group, "per_case": per_case}
    path = os.path.join(os.path.dirname(HERE), "golden", "knn_fp32_distances.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
