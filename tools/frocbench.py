"""Developer tool (GPU box): the CAMELYON16 evaluation mask (froc.evaluation_mask: thresholded exact EDT, hole fill,
8-connected labels, csrc/froc.hip) on a blob mask of a typical level-5 size, against scipy's pipeline on the same mask
(distance_transform_edt + binary_fill_holes + label, what the reference's script runs).  Not a gate.
usage: python tools/frocbench.py [H] [W] [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import froc  # noqa: E402

H = int(sys.argv[1]) if len(sys.argv) > 1 else 7168
W = int(sys.argv[2]) if len(sys.argv) > 2 else 3072
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
rng = np.random.default_rng(0)
mask = np.zeros((H, W), np.uint8)
for _ in range(400):  # elliptic blobs, some with holes, and scattered dots
    r, c, a, b = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, 120)), int(rng.integers(2, 120))
    r0, r1, c0, c1 = max(0, r - a), min(H, r + a + 1), max(0, c - b), min(W, c + b + 1)
    rr, cc = np.ogrid[r0:r1, c0:c1]
    e = ((rr - r) / a) ** 2 + ((cc - c) / b) ** 2
    sub = mask[r0:r1, c0:c1]
    sub[e <= 1] = 255
    if rng.random() < 0.4:
        sub[e <= 0.3] = 0
mask[rng.random((H, W)) < 2e-4] = 255
dev = torch.from_numpy(mask).cuda()
for _ in range(3):
    em = froc.evaluation_mask(dev)
torch.cuda.synchronize()
start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
ts = []
for _ in range(reps):  # each call ends in the .item() of the label count: a device synchronise
    start.record()
    em = froc.evaluation_mask(dev)
    end.record()
    torch.cuda.synchronize()
    ts.append(start.elapsed_time(end))
ts.sort()
print(f"device evaluation mask {H} x {W}: median {ts[len(ts) // 2]:.3f} ms, min {ts[0]:.3f} ms over {reps} calls, {em.n} labels")
t = time.perf_counter()
m = froc.region_moments(em)
torch.cuda.synchronize()
print(f"region moments + ITC list: {(time.perf_counter() - t) * 1e3:.2f} ms, {len(froc.computeITCList(em))} ITC of {em.n}")
try:
    import froc_cpu  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
try:
    import froc_cpu

    t = time.perf_counter()
    ref = froc_cpu.evaluation_mask(mask)
    dt = time.perf_counter() - t
    print(f"scipy pipeline (1 host thread): {dt * 1e3:.0f} ms; labels equal: {bool(np.array_equal(ref, em.numpy()))}")
except ImportError as e:
    print(f"scipy not importable ({e}): no host comparison")
