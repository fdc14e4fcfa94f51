"""Developer tool (GPU box): what the Macenko stain normalisation (stain.py, csrc/stain.hip, --stain_norm macenko) costs.
On a synthetic slide it times
  * the fit on the coarsest level, stage by stage and as a whole (three reductions over the level, three one-workgroup stages);
  * the pixel map of every level, in place, beside a plain device copy of the same level (the yardstick: it moves the same bytes),
and prints the effective bandwidth of both (bytes read + bytes written).  Medians of `reps` runs after a warm-up, the device
synchronised on both sides of every timed region, map and copy alternated run by run.  Not a gate.
usage: python tools/stainbench.py [W] [H] [reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import extract, stain, synth  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
W = int(argv[0]) if len(argv) > 0 else 20000
H = int(argv[1]) if len(argv) > 1 else 16000
reps = max(5, int(argv[2])) if len(argv) > 2 else 5


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


slide = extract.DeviceSlide(synth.build_pyramid(synth.synth_level0(W, H, seed=2, device="cuda"), 4), name="bench")
norm = stain.StainNorm()
lc = len(slide.levels) - 1
level, width = slide.levels[lc], slide.level_dimensions[lc][0]
bq, pm = stain.beta_q(norm.beta), stain.alpha_permille(norm.alpha)


def whole_fit():
    slide.__dict__.pop("_stain_fits", None)  # the fit is cached per slide: time making it
    return norm.fit(slide)


fit = whole_fit()
print(f"== {W} x {H}, level {lc} {width} x {level.shape[0]} ({level.numel() / 1e6:.1f} MB): {fit.report()}")
stages = alternate({
    "moments": lambda: stain.moments(level, width, bq),
    "basis": lambda: stain.basis(fit.moments),
    "angle histogram": lambda: stain.angle_hist(level, width, bq, fit.basis),
    "vectors": lambda: stain.vectors(fit.angle_hist, fit.basis, fit.basis_status, pm),
    "concentration histograms": lambda: stain.conc_hist(level, width, bq, fit.he_p),
    "matrix": lambda: stain.matrix(fit.conc_hist, fit.he_p, fit.vec_status),
    "whole fit": whole_fit,
})
print("   fit stages, median ms (allocation and launch included): " + ", ".join(f"{k} {v:.3f}" for k, v in stages.items()))
total = {"apply": 0.0, "copy": 0.0}
for l, (img, (w, _)) in enumerate(zip(slide.levels, slide.level_dimensions)):
    other = torch.empty_like(img)
    r = alternate({"apply": lambda: stain.apply(img, w, fit.m_maxc, fit.status),  # in place, again and again: the cost is the same
                   "apply into another buffer": lambda: stain.apply(img, w, fit.m_maxc, fit.status, out=other),
                   "copy": lambda: other.copy_(img)})
    gb = 2 * img.numel() / 1e9
    print(f"   level {l} ({img.numel() / 1e6:.1f} MB): apply in place {r['apply']:.3f} ms ({gb / r['apply'] * 1e3:.0f} GB/s), into another buffer "
          f"{r['apply into another buffer']:.3f} ms, device copy {r['copy']:.3f} ms ({gb / r['copy'] * 1e3:.0f} GB/s)")
    total["apply"] += r["apply"]
    total["copy"] += r["copy"]
    del other
print(f"   all levels: apply {total['apply']:.3f} ms, device copy {total['copy']:.3f} ms; whole fit {stages['whole fit']:.3f} ms")
