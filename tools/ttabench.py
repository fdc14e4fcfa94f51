"""Developer tool (GPU box): what the test-time augmentation of the detector costs (tta.py, csrc/tta.hip).  Not a gate.

(a) hipac_tta_view per view on n patches (default 8 192 = one forward slice, 1.23 GB) against a device-to-device copy of the
    same bytes (torch.Tensor.copy_): each byte is read once and written once in both, so the copy is the yardstick.  Each
    view's time is also stated as a share of the trunk's forward of the same slice (26 ms at the README's rate).
(b) detect.detect_slide with tta="d4" against tta="none" on a synthetic slide (default 20 000 x 16 000) at all four levels,
    and the share of the difference that the view kernel and the reduction account for (timed on their own over the same
    number of windows).

Median of 7, the modes alternated, the device synchronised around every timed region.
usage: python tools/ttabench.py [n] [W] [H]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import capi, detect, extract, synth, tta  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
W = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
H = int(sys.argv[3]) if len(sys.argv) > 3 else 16000
REPS, FORWARD_MS_PER_8192 = 7, 26.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def medians(modes):
    """name -> median ms over REPS rounds; every round runs every mode once, in order (the modes alternate)."""
    for fn in modes.values():  # warm-up: allocations, code objects
        fn()
    ts = {k: [] for k in modes}
    for _ in range(REPS):
        for k, fn in modes.items():
            ts[k].append(timed(fn))
    return {k: sorted(v)[REPS // 2] for k, v in ts.items()}


# ---- (a) the view kernel against a copy ------------------------------------------------------------------------------
x = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, device="cuda")
out = torch.empty_like(x)
gb = x.numel() / 1e9
modes = {"copy": lambda: out.copy_(x)}
for v in range(8):
    modes[f"view {v}"] = lambda v=v: tta.view(x, v, out=out)
m = medians(modes)
fwd = FORWARD_MS_PER_8192 * n / 8192
print(f"(a) n = {n} patches, {gb:.2f} GB read and {gb:.2f} GB written per call; forward of the slice ~{fwd:.1f} ms")
print(f"    copy_   {m['copy']:7.3f} ms  {2 * gb / m['copy']:6.2f} TB/s")
for v in range(8):
    t = m[f"view {v}"]
    print(f"    view {v}  {t:7.3f} ms  {2 * gb / t:6.2f} TB/s  {t / m['copy']:5.2f} x copy  {100 * t / fwd:5.1f} % of the forward")
del x, out
torch.cuda.empty_cache()

# ---- (b) detect_slide with and without the views ---------------------------------------------------------------------
LEVELS = (0, 1, 2, 3)
slide = extract.DeviceSlide.synthetic(W, H, seed=5)
net = capi.PackedResNet18(synth.seeded_resnet18_state_dict(0, num_classes=2), precision="bf16")
res = {}


def run(mode):
    res[mode] = detect.detect_slide(slide, net, levels=LEVELS, tta=mode)


m = medians({"none": lambda: run("none"), "d4": lambda: run("d4")})
nw = res["d4"].probs.shape[0]
print(f"(b) {W} x {H}, levels {LEVELS}: {nw} windows; none {m['none']:.1f} ms, d4 {m['d4']:.1f} ms = {m['d4'] / m['none']:.2f} x")
# the TTA's own device code over the same number of windows: seven views of every slice, and the reduction in place of the probabilities
buf = net.batch_buffer(nw, slide.device)
lg = torch.randn((8, nw, 2), device="cuda")


def seven_views():
    for lo in range(0, nw, 8192):
        end = min(nw, lo + 8192)
        for v in range(1, 8):
            tta.view(buf[lo:end], v, out=net.view_buffer(end - lo, slide.device))


k = medians({"views": seven_views, "reduce": lambda: tta.reduce(lg, want_range=True), "probs": lambda: detect.tumor_probs(lg[0])})
extra = m["d4"] - m["none"]
own = k["views"] + k["reduce"] - k["probs"]
print(f"    seven views of {nw} windows {k['views']:.2f} ms, reduce {k['reduce']:.3f} ms (probs alone {k['probs']:.3f} ms): "
      f"{own:.2f} ms = {100 * own / extra:.1f} % of the {extra:.1f} ms the views add; the rest is seven more forwards")
