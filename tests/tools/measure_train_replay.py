"""How far the stage-by-stage replay of the native training step (oracle/train_replay.py) moves when its convolutions
and sums run in float32 instead of float64 -- the distance summation order alone leaves between two correct
implementations of the driver -- on exactly the cases of tests/test_gpu_train_stages.py (CPU only).  Writes
tests/golden/train_replay_distances.json:

    {"scale_exp": {batch: k},                      dfeats = 2^k randn, chosen here from the float16 emulation
     "conditions": {batch: {...}},                 what the choice was checked against (below)
     "cases": {"<precision>-B<batch>[-acc]": {tensor: max|f32 - f64| / max|f64|, "<conv weight>@tap": worst filter tap}},
     "per_storage": {precision: {tensor: the largest figure over that precision's cases}}}

Both replays start from the SAME maps (``emulate_forward`` with the precision's storage type) and round every gradient
map to that type where the device does; only the accumulation type differs.  The GPU test gates the device's distance
from the float64 replay of ITS maps at 10 x the per_storage figure (factor and rule of tests/test_gpu_mil_train.py: the
largest figure over the cases that share the computation's arithmetic, since one case's figure is one draw of rounding
noise); nothing is pooled across storage types.

Condition on the inputs.  The float16 gradient maps must sit inside the format: the loss scale 2^k is chosen per batch
so that, in the float16 emulation (float64 accumulation), no element of any gradient map exceeds 65504 / 4 and at most
0.1 % of the non-zero elements of any gradient map lie below 2^-14 (float16's smallest normal number).  k is the largest
exponent that leaves a factor 8 below 65504 in a float32 probe without gradient rounding; both conditions are then
ASSERTED on the emulation itself, for every case and loss gradient, and the shares found are written out.  Every case of
this file satisfies both (largest share 2.3e-4, largest magnitude 8148); were a batch ever to have no such k the assertion
stops the tool, and that batch's tensors would need an absolute gate instead -- nothing is excluded silently.

    python tests/tools/measure_train_replay.py
"""
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import train_stage_cases as cases  # noqa: E402
from oracle import train_replay as R  # noqa: E402

F16_MAX, F16_MIN_NORMAL, SHARE = 65504.0, 2.0 ** -14, 1e-3


def map_figures(gm):
    """per gradient map: (largest magnitude, share of the non-zero elements below float16's smallest normal)."""
    out = {}
    for k, v in gm.items():
        a = v.abs().flatten()
        nz = a[a > 0]
        out[k] = (float(a.max()), float((nz < F16_MIN_NORMAL).double().mean()) if nz.numel() else 0.0)
    return out


def choose_scale(maps16, sd, batch):
    probe = {}
    R.replay_backward(maps16, sd, cases.make_dfeats(batch, 0), None, torch.float32, grad_maps=probe)
    top = max(float(v.abs().max()) for v in probe.values())
    return int(math.floor(math.log2(F16_MAX / 8 / top)))


def main():
    sd = cases.make_state_dict()
    out = {"scale_exp": {}, "conditions": {}, "cases": {}, "per_storage": {}}
    for batch in cases.BATCHES:
        x = cases.make_input(batch)
        maps = {p: R.emulate_forward(x, sd, st) for p, st in cases.STORAGE.items()}
        k = choose_scale(maps["fp16"], sd, batch)
        out["scale_exp"][str(batch)] = k
        runs = [(f"B{batch}", (0,))] + ([(f"B{batch}-acc", (0, 1))] if batch == cases.ACC_BATCH else [])
        for prec, st in cases.STORAGE.items():
            for tag, which in runs:
                g = {}
                for acc in (torch.float64, torch.float32):
                    tot = None
                    for wdf in which:
                        gm = {}
                        r = R.replay_backward(maps[prec], sd, cases.make_dfeats(batch, k, wdf), st, acc, grad_maps=gm)
                        tot = r if tot is None else {n: tot[n] + r[n] for n in r}
                        if prec == "fp16" and acc == torch.float64:
                            figs = map_figures(gm)
                            worst_top = max(v[0] for v in figs.values())
                            worst_share = max(figs.items(), key=lambda kv: kv[1][1])
                            ok = worst_top <= F16_MAX / 4 and worst_share[1][1] <= SHARE
                            out["conditions"][f"{tag}-df{wdf}"] = {
                                "satisfied": ok, "largest_magnitude": worst_top, "largest_allowed": F16_MAX / 4,
                                "largest_share_below_2^-14": worst_share[1][1], "in_map": worst_share[0], "share_allowed": SHARE,
                                "maps_failing": sorted(m for m, v in figs.items() if v[0] > F16_MAX / 4 or v[1] > SHARE)}
                            assert ok, (tag, wdf, out["conditions"][f"{tag}-df{wdf}"])
                    g[acc] = tot
                d = cases.tensor_figures(g[torch.float32], g[torch.float64])
                out["cases"][f"{prec}-{tag}"] = d
                agg = out["per_storage"].setdefault(prec, {})
                for n, v in d.items():
                    agg[n] = max(agg.get(n, 0.0), v)
                print(f"{prec}-{tag} scale 2^{k}", {n: f"{v:.1e}" for n, v in d.items() if n.endswith("weight") and "bn" not in n and "downsample.1" not in n}, flush=True)
    path = os.path.join(os.path.dirname(HERE), "golden", "train_replay_distances.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)
    print(json.dumps(out["conditions"], indent=1))


if __name__ == "__main__":
    main()
