"""Developer tool (GPU box): what one training step of the gated MIL model (hipac_mil_gated_train_fwd_bwd,
csrc/mil_gated.hip) costs at the reference dims (F = 512, A = 128, hidden 128, 2 classes), for K = 1 and K = 8 heads, on
two batches: 32 bags of 100 rows (the yaml's batch) and 32 bags of 4 000 rows, the rows read in place through a permuted
index.

The yardstick is the UNGATED step on the same rows and K: hipac_mil_train_fwd_bwd for K = 1, hipac_mil_heads_train_fwd_bwd
for K = 8, both through NativeMILTrainer.forward_backward.  The gate doubles the two MFMA products (X V^T, dH^T X) and leaves
the three other passes as they are, so the ratio gated / ungated should stay below 2.  Median of `reps` runs (7 unless
given) after a warm-up, the device synchronised on both sides of every timed region, the modes alternated run by run.
Prints one JSON line per (batch, K).  Not a gate.
usage: python tools/milgatedbench.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import mil, mil_train  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = max(3, int(argv[0])) if len(argv) > 0 else 7
F, BAGS, SEED = 512, 32, 0

if not torch.cuda.is_available():
    sys.exit("milgatedbench needs a ROCm device: a CPU run says nothing about the kernel")
dev = torch.device("cuda", torch.cuda.current_device())


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for rows_per_bag in (100, 4000):
    n = BAGS * rows_per_bag
    g = torch.Generator().manual_seed(SEED)
    feats = (0.7 * torch.randn(n + 1234, F, generator=g)).to(dev)
    rows = torch.randperm(n + 1234, generator=g)[:n].to(torch.int32)
    offsets = np.arange(BAGS + 1, dtype=np.int64) * rows_per_bag
    labels = torch.arange(BAGS) % 2
    for K in (1, 8):
        torch.manual_seed(SEED)
        gated = mil_train.NativeMILTrainer(mil.MILClassifier(F, 2, "attention", heads=K, gated=True).state_dict(), "attention", dev)
        plain = mil_train.NativeMILTrainer(mil.MILClassifier(F, 2, "attention", heads=K).state_dict(), "attention", dev)
        assert gated.gated and not plain.gated and gated.heads == plain.heads == K
        modes = {"gated_step": lambda: gated.forward_backward(feats, rows, offsets, labels),
                 "ungated_step": lambda: plain.forward_backward(feats, rows, offsets, labels)}
        for fn in modes.values():
            timed(fn)
        ts = {k: [] for k in modes}
        for _ in range(reps):
            for k, fn in modes.items():
                ts[k].append(timed(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        print(json.dumps({"heads": K, "bags": BAGS, "rows_per_bag": rows_per_bag, "feature_dim": F, "reps": reps,
                          "gated_step_ms": round(med["gated_step"], 3), "ungated_step_ms": round(med["ungated_step"], 3),
                          "ratio_gated_over_ungated": round(med["gated_step"] / med["ungated_step"], 2),
                          "all_ms": {k: [round(x, 3) for x in v] for k, v in ts.items()}}), flush=True)
