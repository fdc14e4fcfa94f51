"""Developer tool (GPU box): what --validate (validate.py, csrc/validate.hip) costs on N x 512 synthetic feature rows, beside what
a user without it would run: the float64 restatement of tests/validate_cpu.py on 16 host threads on the same rows, and
scikit-learn where it imports.  It times
  * PCA end to end (column sums, Gram matrix, eigh on the host, projection and class means; the upload is not counted: the
    features are on the device already when they come from --extract_features in the same process, and a PCIe copy is not the
    kernel's doing -- it is printed on its own line),
  * one Newton iteration (one sweep + one weighted Gram + the host solve),
  * the probe end to end (tol 1e-4),
and the Gram kernel and the sweep alone: the Gram's rate as a share of the exact-f32 MFMA peak (157.3 TFLOP/s), counting the
2 N F^2 FLOP of the full product although only the tiles on or above the diagonal are computed (so the share can pass 1) and,
beside it, the FLOP the kernel executes; the sweep's N F 4 bytes as a share of the HBM bandwidth a float4 copy reaches (6.3 TB/s).
Medians of `reps` runs after a warm-up, the device synchronised on both sides of every timed region, device and host modes
alternated run by run.  Not a gate.
usage: python tools/validatebench.py [N] [reps] [--host_reps R] [--sklearn_reps R] [--no_host]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import validate_cpu as cpu  # noqa: E402
from ss25_hierarchical_multiscale_image_classification_amd import validate  # noqa: E402


def flag(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1].startswith("--")]
N = int(pos[0]) if len(pos) > 0 else 1_000_000
reps = int(pos[1]) if len(pos) > 1 else 7
host_reps, sk_reps, no_host = flag("--host_reps", reps), flag("--sklearn_reps", 1), "--no_host" in sys.argv
F, MFMA_F32_PEAK, HBM_COPY = 512, 157.3e12, 6.3e12
torch.set_num_threads(16)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def alternate(fns, counts):
    """{name: median ms} of the callables, run in turn (callable k ``counts[k]`` times in all) after one warm-up of the device ones."""
    ts = {k: [] for k in fns}
    for k, fn in fns.items():
        if k.startswith("device"):
            timed(fn)
    for i in range(max(counts.values())):
        for k, fn in fns.items():
            if i < counts[k]:
                ts[k].append(timed(fn)[0])
    return {k: median(v) for k, v in ts.items() if v}


# two overlapping clusters plus two high-variance directions, as tests/validate_cases.py makes them, drawn on the device
g = torch.Generator(device="cuda").manual_seed(1)
y_dev = (torch.rand(N, device="cuda", generator=g) < 0.4).long()
q, _ = torch.linalg.qr(torch.randn(F, 3, device="cuda", generator=g))
X = 1.0 + 0.5 * torch.randn(N, F, device="cuda", generator=g)
X += 1.5 * (y_dev.float() - 0.5)[:, None] * q[:, 0]
X += 4.0 * torch.randn(N, 1, device="cuda", generator=g) * q[:, 1] + 2.5 * torch.randn(N, 1, device="cuda", generator=g) * q[:, 2]
x, y = X.cpu().numpy(), y_dev.cpu().numpy()
up_ms, _ = timed(lambda: torch.from_numpy(x).to("cuda"))
print(f"== {N} x {F} float32 ({x.nbytes / 1e9:.2f} GB), {reps} runs; host to device copy {up_ms:.1f} ms (not counted below)")

train, test = validate.stratified_split(y, 42)
cw = validate.balanced_class_weights(y[train])
train_dev = torch.from_numpy(train.astype(np.int32)).to("cuda")
cw_dev = torch.tensor(cw, dtype=torch.float32, device="cuda")
coef0, icpt0 = torch.zeros(F, device="cuda"), torch.zeros(1, device="cuda")


def device_newton_iteration():
    sums, d, _ = validate.logistic_sweep(X, y_dev, coef0, icpt0, cw_dev, rows=train_dev, check_rows=False)
    h = sums.cpu().numpy().astype(np.float64)
    H = np.empty((F + 1, F + 1))
    H[:F, :F] = validate.gram(X, rows=train_dev, w=d, check_rows=False).cpu().numpy().astype(np.float64) + np.eye(F)
    H[:F, F] = H[F, :F] = h[F:2 * F]
    H[F, F] = h[2 * F + 1]
    return np.linalg.solve(H, -np.concatenate([h[:F], [h[2 * F]]]))


def host_newton_iteration():
    sw = cpu.sweep(x, y, np.zeros(F), np.zeros(1), cw, rows=train)
    H = np.empty((F + 1, F + 1))
    H[:F, :F] = cpu.gram(x, rows=train, w=sw["d"]) + np.eye(F)
    H[:F, F] = H[F, :F] = sw["curv"][:F]
    H[F, F] = sw["curv"][F]
    return np.linalg.solve(H, -sw["grad"])


fits = {}


def device_probe():
    fits["device"] = validate.fit_probe(X, y_dev, train_dev, cw, 1.0, 1e-4)


def host_probe():
    fits["host"] = cpu.newton(x, y, train, cw, tol=1e-4)


def line(what, r):
    dev_ms = r["device"]
    rest = ", ".join(f"{k} {v:.1f} ms ({v / dev_ms:.1f} x)" for k, v in r.items() if k != "device")
    print(f"   {what}: device {dev_ms:.2f} ms" + (f"; {rest}" if rest else ""))


hc = 0 if no_host else host_reps
line("PCA end to end", alternate({"device": lambda: validate.pca_device(X, y_dev), "host float64, 16 threads": lambda: cpu.pca(x, y)},
                                 {"device": reps, "host float64, 16 threads": hc}))
line("one Newton iteration", alternate({"device": device_newton_iteration, "host float64, 16 threads": host_newton_iteration},
                                       {"device": reps, "host float64, 16 threads": hc}))
probe = {"device": device_probe, "host float64, 16 threads": host_probe}
counts = {"device": reps, "host float64, 16 threads": hc}
try:
    from sklearn.linear_model import LogisticRegression

    if not no_host and sk_reps > 0:
        xt, yt = x[train], y[train]
        probe["scikit-learn L-BFGS, float32 input"] = lambda: fits.__setitem__(
            "sklearn", LogisticRegression(max_iter=1000, class_weight="balanced").fit(xt, yt))
        counts["scikit-learn L-BFGS, float32 input"] = sk_reps
except ImportError:
    print("   scikit-learn does not import here: no L-BFGS figure")
line("probe end to end", alternate(probe, counts))
f = fits["device"]
print(f"   device probe: {f['iterations']} Newton iterations, gradient {f['gradient_norm']:.2e}, converged {f['converged']}"
      + (f"; host: {fits['host']['iterations']} iterations" if "host" in fits else ""))

_, d, _ = validate.logistic_sweep(X, y_dev, coef0, icpt0, cw_dev)
kern = alternate({"device gram": lambda: validate.gram(X, w=d), "device gram, centred": lambda: validate.gram(X, c=coef0),
                  "device sweep": lambda: validate.logistic_sweep(X, y_dev, coef0, icpt0, cw_dev),
                  "device colsum": lambda: validate.colsum(X)}, {k: reps for k in ("device gram", "device gram, centred", "device sweep", "device colsum")})
full = 2.0 * N * F * F
tiles = (F // 32) * (F // 32 + 1) // 2
done = 2.0 * N * tiles * 1024
for k in ("device gram", "device gram, centred"):
    s = kern[k] * 1e-3
    print(f"   {k[7:]} {kern[k]:.3f} ms: {full / s / 1e12:.1f} TFLOP/s of the full product = {full / s / MFMA_F32_PEAK:.2f} of the exact-f32 MFMA "
          f"peak; executed (tiles on or above the diagonal) {done / s / 1e12:.1f} TFLOP/s = {done / s / MFMA_F32_PEAK:.2f}")
for k in ("device sweep", "device colsum"):
    s = kern[k] * 1e-3
    print(f"   {k[7:]} {kern[k]:.3f} ms: {N * F * 4 / s / 1e12:.2f} TB/s = {N * F * 4 / s / HBM_COPY:.2f} of the 6.3 TB/s a float4 copy reaches")
