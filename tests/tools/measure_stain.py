"""Measure how far the integer restatement of the Macenko fit (tests/stain_cpu.py) is from the textbook float64 algorithm, once, on
the CPU, and record it in tests/golden/stain_distances.json (tests/test_stain_host.py allows 2 x the recorded angle, maxC difference
and share of differing pixels on other seeds, and requires the recorded largest pixel difference).

    python tests/tools/measure_stain.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import stain_cases  # noqa: E402


def main():
    per_seed = {str(s): stain_cases.distances(stain_cases.two_stain_image(s)) for s in stain_cases.SEEDS}
    rec = {"what": "restatement (tests/stain_cpu.py) against textbook float64 Macenko, seeded two-stain images of 400 x 500 pixels, alpha 1, "
                   "beta 0.15; the largest value over the seeds",
           "seeds": list(stain_cases.SEEDS),
           "angle_deg": max(d["angle_deg"] for d in per_seed.values()),
           "dmaxc": max(d["dmaxc"] for d in per_seed.values()),
           "max_pixel_diff": max(d["max_pixel_diff"] for d in per_seed.values()),
           "share_differing": max(d["share_differing"] for d in per_seed.values()),
           "per_seed": per_seed}
    path = os.path.join(os.path.dirname(HERE), "golden", "stain_distances.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
