"""Measures, ON THE CPU, the d of oracle/pair_replay.py's tolerance b = FACTOR d max|ref| and writes
tests/golden/pair_replay_distances.json.

d of a stage = the largest max|v - ref| / max|ref| over the cases below (d_rms, per slice kind: the largest root mean square of v - ref over one
channel, over one row, over one column, PR.slice_rms, over max|ref|), v = the UNROUNDED float32 epilogue value of the
float32 stand-in (tests/pair_replay_cases.py: torch float32 convolutions, the product kinds summed separately), ref = the
float64 replay of the same conv from the stand-in's own operand planes.  That is the distance an fp32 sum in another order
leaves; no device figure enters.  Also recorded: the stand-in's rate m / T of the ``tie`` check per case (the check's gate is
T / 16, see the oracle's docstring).

usage: python tests/tools/measure_pair_replay.py [--check]     (--check: measure and compare with the committed file, within a factor 2)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_replay_cases as cases  # noqa: E402
from oracle import pair_replay as PR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pair_replay_distances.json")
# (weights, stem form, patches): the CPU cases of tests/test_oracle_pair_replay.py
CHECK_FACTOR = 2.0  # --check: how far a re-measured figure may lie from the committed one
CASES = (("plain", "u8_strip", 3), ("rescaled", "u8_strip", 3), ("plain", "nchw_f32", 2))


def measure() -> dict:
    torch.manual_seed(0)
    out = {"how": "tests/tools/measure_pair_replay.py on the CPU: per stage the largest max|v - ref| / max|ref| of the float32 stand-in's "
                  "unrounded epilogue value (\"rms\": per slice kind -- ch, row, col -- of its largest root mean square over one such slice) against the float64 replay from the stand-in's own planes, over `cases` and their images "
                  "(one image at a time); the oracle's tolerance is factor * d * max|ref|",
           "factor": PR.FACTOR, "cases": [list(c) for c in CASES], "torch": torch.__version__, "tie_rate": {}}
    for mode in PR.MODES:
        d: dict = {}
        r: dict = {}
        rates = []
        for weights, stem, n in CASES:
            W = PR.pack(cases.state_dict(weights))
            u8 = cases.patches(n)
            inp = cases.normalized(u8) if stem == "nchw_f32" else u8
            dev = cases.to64(cases.standin_forward(mode, inp, W, stem=stem))
            for i in range(n):
                one = PR.slice_image(dev, i)
                for k, (v, v_rms) in cases.standin_distances(mode, one, W, stem).items():
                    d[k] = max(d.get(k, 0.0), v)
                    r[k] = {q: max(r.get(k, {}).get(q, 0.0), x) for q, x in v_rms.items()}
                if mode == "fp16q8":
                    for b in range(7):
                        t = PR.tie_statistic(one["out"][b])
                        if t["T"] >= PR.TIE_MIN:
                            rates.append(t["m"] / t["T"])
        out[mode] = {"max": {k: float(f"{v:.4g}") for k, v in sorted(d.items())}, "rms": {k: {q: float(f"{x:.4g}") for q, x in v.items()} for k, v in sorted(r.items())}}
        if rates:
            out["tie_rate"] = {"min": float(f"{min(rates):.3g}"), "max": float(f"{max(rates):.3g}"), "maps": len(rates)}
    return out


if __name__ == "__main__":
    res = measure()
    if "--check" in sys.argv:
        # another CPU or torch build sums float32 in another order: the figures agree within CHECK_FACTOR, not digit for digit
        old = json.load(open(OUT))
        ok = True
        for mode in PR.MODES:
            rows = [("max", k, v, old[mode]["max"][k]) for k, v in res[mode]["max"].items()]
            rows += [("rms " + q, k, x, old[mode]["rms"][k][q]) for k, v in res[mode]["rms"].items() for q, x in v.items()]
            for kind, k, new, was in rows:
                good = was / CHECK_FACTOR <= new <= was * CHECK_FACTOR
                ok &= good
                print(f"{mode:7s} {kind:8s} {k:26s} measured {new:.4g}  committed {was:.4g}{'' if good else '  <-- differs by more than a factor ' + str(CHECK_FACTOR)}")
        sys.exit(0 if ok else 1)
    with open(OUT, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
