"""Developer tool (GPU box): how fast a tiled pyramidal TIFF gets into HBM (tiff_pyramid.TiffPyramid.to_device_levels:
tiles decoded on host threads, copied band by band) next to the scan of the same slide.
usage: python tools/tiffbench.py [side] [compression: jpeg|deflate|none|lzw] [workers] [--compression lzw|deflate]
With LZW the tool compares the device decoder (csrc/lzw.hip) with the host decoder on ``workers`` threads on the same file:
median of 5 loads each, modes alternated (the writer's LZW encoder is plain Python: keep ``side`` small, default 2048).
``--compression deflate`` compares csrc/deflate.hip with zlib on ``workers`` threads in the same way (deflate as a positional
argument times from_tiff and the scan, as before)."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import capi, extract, synth, tiff_pyramid  # noqa: E402

argv = list(sys.argv[1:])
flag = None
if "--compression" in argv:
    k = argv.index("--compression")
    flag = argv[k + 1]
    del argv[k:k + 2]
comp = flag or (argv[1] if len(argv) > 1 else "jpeg")
side = int(argv[0]) if argv else (2048 if comp == "lzw" else 20000)
workers = int(argv[2]) if len(argv) > 2 else 16
l0 = synth.synth_level0(side, side, seed=2, device="cuda")
levels = [t.cpu().numpy() for t in synth.build_pyramid(l0, 4)]
path = os.path.join(tempfile.mkdtemp(prefix="hipac_tiff_"), "slide.tif")
t = time.perf_counter()
tiff_pyramid.write_tiled_tiff(path, levels, tile=512, compression=comp)
print(f"wrote {path}: {os.path.getsize(path) / 1e6:.0f} MB in {time.perf_counter() - t:.1f} s")
del l0, levels
if comp == "lzw" or flag == "deflate":
    import statistics

    times = {True: [], False: []}
    tp = tiff_pyramid.TiffPyramid(path)
    px = sum(w * h for w, h in tp.level_dimensions)
    switch = "device_lzw" if comp == "lzw" else "device_deflate"
    tp.to_device_levels("cuda", **{switch: True})  # the first call loads the code object
    for rep in range(5):
        for on_device in (True, False):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = tiff_pyramid.TiffPyramid(path).to_device_levels("cuda", workers=workers, **{switch: on_device})
            torch.cuda.synchronize()
            times[on_device].append(time.perf_counter() - t)
            del out
    for on_device, name in ((True, "device"), (False, f"host, {workers} threads")):
        m = statistics.median(times[on_device])
        print(f"to_device_levels ({comp}, {name}): median of 5 {m:.3f} s = {px / 1e6 / m:.1f} Mpx/s  {[round(x, 3) for x in times[on_device]]}")
    sys.exit(0)
for rep in range(2):
    t = time.perf_counter()
    slide = extract.DeviceSlide.from_tiff(path, workers=workers)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    px = sum(w * h for w, h in slide.level_dimensions)
    print(f"from_tiff ({comp}, {workers} threads): {dt:.2f} s = {px * 3 / dt / 1e9:.2f} GB/s of decoded pixels, {px / 1e6 / dt:.0f} Mpx/s")
net = capi.PackedResNet18(synth.seeded_resnet18_state_dict(0, num_classes=2), precision="bf16")
for rep in range(2):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f, l, p, m = extract.score_slide(slide, net, levels=(0, 1, 2, 3))
    torch.cuda.synchronize()
    print(f"score_slide: {time.perf_counter() - t:.3f} s, {f.shape[0]} kept windows")
