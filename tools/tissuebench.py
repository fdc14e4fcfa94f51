"""Developer tool (GPU box): what the Otsu tissue mask (tissue.py, csrc/tissue.hip, --tissue_filter otsu) costs and saves.
On a dense synthetic slide (six blobs) and a sparse one (n_blobs = 1) of the same size it times
  * the mask stages alone (thumbnail + histogram, Otsu, clean-up, table; the window decisions of one level);
  * the level-3 dense scan of --detect_cell 32 (stride 4: the per-window path) with `white` and with `otsu`;
  * the whole detection of --patch_level all at the default cell, both ways,
and prints kept / total windows beside the times.  Medians of `reps` runs after a warm-up, the device synchronised on both
sides of every timed region, the two modes alternated run by run.  Not a gate.
usage: python tools/tissuebench.py [W] [H] [reps] [--no-dense]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import capi, detect, extract, synth, tissue  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
W = int(argv[0]) if len(argv) > 0 else 50000
H = int(argv[1]) if len(argv) > 1 else 50000
reps = max(5, int(argv[2])) if len(argv) > 2 else 5
dense_scan = "--no-dense" not in sys.argv


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def alternate(fns):
    """{name: median ms} of the callables, run in turn ``reps`` times after one warm-up each."""
    for fn in fns.values():
        timed(fn)
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn)[0])
    return {k: median(v) for k, v in ts.items()}


def fresh_mask(slide):
    slide.__dict__.pop("_tissue_masks", None)  # the mask is cached per slide: time making it
    return flt.mask(slide)


net = capi.PackedResNet18(synth.seeded_resnet18_state_dict(0, num_classes=2), precision="bf16")
flt = tissue.TissueFilter()
for label, blobs in (("dense slide (6 blobs)", 6), ("sparse slide (1 blob)", 1)):
    slide = extract.DeviceSlide(synth.build_pyramid(synth.synth_level0(W, H, seed=2, n_blobs=blobs, device="cuda"), 4), name=label)
    w3, h3 = slide.level_dimensions[3]
    tm = fresh_mask(slide)
    print(f"== {label}: {W} x {H}, level 3 {w3} x {h3} ({slide.levels[3].numel() / 1e6:.1f} MB), mask {tm.mask.shape[1]} x {tm.mask.shape[0]}; "
          f"{tm.report()}")
    xy3 = torch.from_numpy(extract.window_grid(w3, h3, 3, 4)[2]).to(slide.device)
    stages = alternate({
        "thumbnail + histogram": lambda: tissue.thumbnail(slide.levels[3], w3, 4),
        "otsu": lambda: tissue.otsu(tm.hist, 16),
        "clean-up": lambda: tissue.clean_mask(tm.sat, tm.thresholds, 1, True),
        "table": lambda: tissue.integral(tm.mask),
        "whole mask": lambda: fresh_mask(slide),
        f"keep of {xy3.shape[0]} windows": lambda: tm.window_keep(xy3, 3, 0.05),
    })
    print("   mask stages, median ms (allocation and launch included): " + ", ".join(f"{k} {v:.3f}" for k, v in stages.items()))
    gbs = slide.levels[3].numel() / 1e9 / (stages["thumbnail + histogram"] / 1e3)
    print(f"   thumbnail reads the level at {gbs:.0f} GB/s")

    def kept(windows):
        return f"{int(windows.keep.sum())}/{windows.xy.shape[0]}"

    if dense_scan:
        r = alternate({"white": lambda: extract.LevelWindows(slide, 3, stride=4), "otsu": lambda: extract.LevelWindows(slide, 3, stride=4, tissue=flt)})
        lw_w, lw_o = extract.LevelWindows(slide, 3, stride=4), extract.LevelWindows(slide, 3, stride=4, tissue=flt)
        print(f"   level-3 window decisions + resampling at stride 4 (--detect_cell 32): white {r['white']:.1f} ms (kept {kept(lw_w)}), "
              f"otsu {r['otsu']:.1f} ms (kept {kept(lw_o)})")
        del lw_w, lw_o
    r = alternate({"white": lambda: detect.detect_slide(slide, net), "otsu": lambda: detect.detect_slide(slide, net, tissue=flt)})
    n_w, n_o = detect.detect_slide(slide, net).probs.shape[0], detect.detect_slide(slide, net, tissue=flt).probs.shape[0]
    print(f"   detection, levels 0-3, cell 224: white {r['white']:.1f} ms ({n_w} windows scored), otsu {r['otsu']:.1f} ms ({n_o} windows scored)")
    del slide, tm
    torch.cuda.empty_cache()
