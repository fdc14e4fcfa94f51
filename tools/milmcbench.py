"""Developer tool (GPU box): what the Monte-Carlo dropout forward of the MIL head (mil_dropout.mc_forward,
csrc/mil_dropout.hip) costs on one slide-sized workload: a seeded 40 000 x 512 feature matrix in 8 bags, T = 100 samples,
p = 0.5, attention pooling at the reference dims (A = 128, hidden 128, 2 classes).

The yardstick is T back-to-back calls of the existing deterministic forward (capi.mil_forward -> hipac_mil_forward) on the
same bags: the least a host loop over the samples could cost, before it even makes its masked copies of the features.
Median of `reps` runs after a warm-up, the device synchronised on both sides of every timed region, the two modes
alternated run by run; allocation and launch are inside the timed region on both sides.  Prints one JSON line.  Not a gate.
usage: python tools/milmcbench.py [rows] [bags] [T] [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import capi, mil, mil_dropout  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(argv[0]) if len(argv) > 0 else 40000
BAGS = int(argv[1]) if len(argv) > 1 else 8
T = int(argv[2]) if len(argv) > 2 else 100
reps = max(5, int(argv[3])) if len(argv) > 3 else 5
F, P, SEED = 512, 0.5, 0

if not torch.cuda.is_available():
    sys.exit("milmcbench needs a ROCm device: a CPU run says nothing about the kernel")
dev = torch.device("cuda", torch.cuda.current_device())
torch.manual_seed(SEED)
model = mil.MILClassifier(F, 2, "attention")
sd = {k: v.detach().to(dev, torch.float32).contiguous() for k, v in model.state_dict().items()}
feats = (0.7 * torch.randn(N, F, generator=torch.Generator().manual_seed(SEED))).to(dev)
offsets = torch.from_numpy(np.linspace(0, N, BAGS + 1).astype(np.int64))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fused():
    return mil_dropout.mc_forward(sd, "attention", feats, offsets, P, SEED, T)


def host_loop():
    return [capi.mil_forward(sd, "attention", feats, offsets, want_attn=False)[0] for _ in range(T)]


modes = {"mc_forward": fused, "mil_forward_x_T": host_loop}
for fn in modes.values():
    timed(fn)
ts = {k: [] for k in modes}
for _ in range(reps):
    for k, fn in modes.items():
        ts[k].append(timed(fn)[0])
med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
flop = 2.0 * T * N * F * 128  # the X V^T products alone
print(json.dumps({"rows": N, "bags": BAGS, "feature_dim": F, "samples": T, "p": P, "reps": reps,
                  "mc_forward_ms": round(med["mc_forward"], 3), "mil_forward_x_T_ms": round(med["mil_forward_x_T"], 3),
                  "ratio": round(med["mil_forward_x_T"] / med["mc_forward"], 2),
                  "mc_forward_all_ms": [round(v, 3) for v in ts["mc_forward"]],
                  "mil_forward_x_T_all_ms": [round(v, 3) for v in ts["mil_forward_x_T"]],
                  "mc_forward_xv_tflops": round(flop / med["mc_forward"] / 1e9, 2)}))
