"""Measure how far the integer restatement of the HED stain augmentation (tests/augment_hed_cpu.py: quantised optical densities,
the table inverse) is from the textbook float64 formula, once, on the CPU, and record it in
tests/golden/augment_hed_distances.json (tests/test_augment_hed_host.py gates at the recorded figures without a margin: both
sides are deterministic host code).

    python tests/tools/measure_augment_hed.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import augment_hed_cpu as cpu  # noqa: E402


def main():
    per_sigma = cpu.distances()
    rec = {"what": "restatement (tests/augment_hed_cpu.py) against v' = clip(rint(256 exp(-(od A^T + b)) - 1)), od = ln(256 / (v + 1)): "
                   f"{cpu.N_COLOURS} seeded random colours and {cpu.N_COLOURS} H&E-like colours under {cpu.N_MAPS} maps per sigma; levels "
                   "of 0..255 and the share of bytes that differ",
           "sigmas": list(cpu.SIGMAS),
           "max_level_diff": max(d["max_level_diff"] for d in per_sigma.values()),
           "share_differing": max(d["share_differing"] for d in per_sigma.values()),
           "per_sigma": per_sigma}
    path = os.path.join(os.path.dirname(HERE), "golden", "augment_hed_distances.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
