"""Developer tool (GPU box): what the device PNG encoder (png_encode.py, csrc/png_encode.hip, --png_encoder device) buys over the
host leg of --write_png.  On one synthetic level of smooth, H&E-like content with a white share (noise would only measure the
stored path) it encodes the windows of a P = 224 grid and of a P = 1792 grid
  * on the device: windows -> file bytes in host memory, the copy included (png_encode.iter_encoded);
  * on the host: today's leg, one device-to-host copy and one Pillow save into memory per window, on 16 host threads;
  * the device leg's kernels alone (png_encode.encode_windows: buffers allocated, both kernels run, the files left in HBM),
and prints MB/s of raw pixels and the size of the files relative to the raw pixels for both.  Medians of `reps` runs after a
warm-up, the two legs alternated run by run, the device synchronised on both sides of every timed region.  The file writes
themselves are not measured.  Not a gate.
usage: python tools/pngbench.py [SIDE] [reps]"""
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import png_encode  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
SIDE = int(argv[0]) if len(argv) > 0 else 9000
reps = max(5, int(argv[1])) if len(argv) > 1 else 5
THREADS = 16


def smooth_level(side, white_share=0.3, seed=2):
    """uint8[side, side, 3] on the device: low-frequency colour fields, fine grain, white beyond a wavy edge."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rng = np.random.RandomState(seed)
    yy = torch.arange(side, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(side, device="cuda", dtype=torch.float32)[None, :]
    f = torch.zeros((side, side), device="cuda")
    for _ in range(6):
        kx, ky, ph = rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(0, 6.28)
        f += torch.sin(kx * xx + ky * yy + ph)
    f = (f - f.min()) / (f.max() - f.min())
    img = torch.stack([205 - 70 * f, 150 - 90 * f, 200 - 50 * f], -1)
    img += 2.0 * torch.randn(img.shape, generator=g, device="cuda")
    img = img.clamp_(0, 255).round_().to(torch.uint8)
    edge = xx + 0.3 * yy + 300 * torch.sin(yy / 700.0)
    img[edge > (1 - white_share) * 1.3 * side] = 255
    return img.contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


level = smooth_level(SIDE)
print(f"== level {SIDE} x {SIDE} ({level.numel() / 1e6:.0f} MB), smooth content, white share {float((level == 255).all(2).float().mean()):.2f}; "
      f"median of {reps}, legs alternated")
for P in (224, 1792):
    xy = np.array([(x, y) for y in range(0, SIDE, P) for x in range(0, SIDE, P)], np.int32)
    raw_mb = len(xy) * P * P * 3 / 1e6

    def device_leg():
        return [f for _, files in png_encode.iter_encoded(level, SIDE, SIDE, xy, P) for f in files]

    def host_one(pt):
        x, y = int(pt[0]), int(pt[1])
        canvas = np.full((P, P, 3), 255, np.uint8)
        pw, ph = min(P, SIDE - x), min(P, SIDE - y)
        canvas[:ph, :pw] = level[y:y + ph, x:x + pw].cpu().numpy()
        b = io.BytesIO()
        Image.fromarray(canvas, "RGB").save(b, "PNG")
        return b.getvalue()

    def host_leg():
        with ThreadPoolExecutor(THREADS) as ex:
            return list(ex.map(host_one, xy))

    def kernels_only():
        png_encode.encode_windows(level, SIDE, SIDE, xy, P)  # the files stay in HBM: no copy, no host work behind the launches
        return []

    legs = {"device": device_leg, "host": host_leg, "kernels": kernels_only}
    outs = {k: timed(fn)[1] for k, fn in legs.items()}  # warm-up
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ts[k].append(timed(fn)[0])
    a = np.asarray(Image.open(io.BytesIO(outs["device"][len(xy) // 2])))
    b = np.asarray(Image.open(io.BytesIO(outs["host"][len(xy) // 2])))
    assert np.array_equal(a, b), "device and host files decode to different pixels"
    size = {k: sum(len(f) for f in v) for k, v in outs.items()}
    size["kernels"] = size["device"]
    print(f"   P = {P}: {len(xy)} windows, {raw_mb:.0f} MB raw")
    for k in legs:
        ms = median(ts[k])
        print(f"      {k:6s}: {ms:9.1f} ms  {raw_mb / ms * 1e3:8.0f} MB/s of raw pixels; files {size[k] / 1e6:.1f} MB = {size[k] / (raw_mb * 1e6):.3f} of raw")
    print(f"      device / host: {median(ts['host']) / median(ts['device']):.1f}x the speed, {size['device'] / size['host']:.3f} of the size")
