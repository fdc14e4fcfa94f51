"""How far float32 arithmetic itself (torch float32 on the CPU, tests/validate_cpu.py with dt = float32) lands from the
float64 oracle on exactly the inputs of tests/test_gpu_validate.py (CPU only).  Writes
tests/golden/validate_fp32_distances.json:

    {"cases": {kind: {case id: {tensor: max|f32 - f64| / max|f64|}}},
     "per_group": {kind: {"F": {tensor: the largest distance over that group's cases}}},
     "e2e": {"F": {"ratios", "components", "theta", "test_margins", "Z", "class_means": distance, "min_abs_margin",
                   "oracle_accuracy", "oracle_iterations", "fp32_iterations", "eigenvalues": the leading four}},
     "sklearn": {"F": {"theta", "ratios", "components"}}  oracle vs scikit-learn, where it imports: not gated}

kind is "gram" (the column sums and the Gram matrix), "sweep" (the +-80 margins and the one-class case are cases of their F like
the others) or "project".  The GPU test gates every tensor at 10 x the
per-group figure (the rule and the factor of tests/test_gpu_mil_train.py); a group is the cases with the same F, nothing
is pooled across groups.

    python tests/tools/measure_validate_fp32.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import validate_cases as cases  # noqa: E402
import validate_cpu as cpu  # noqa: E402


def main():
    out = {"cases": {"gram": {}, "sweep": {}, "project": {}}, "per_group": {"gram": {}, "sweep": {}, "project": {}}, "e2e": {},
           "sklearn": {}}

    def record(kind, cid, F, d):
        print(kind, cid, {k: f"{v:.2e}" for k, v in d.items()}, flush=True)
        out["cases"][kind][cid] = d
        agg = out["per_group"][kind].setdefault(cases.group_key(F), {})
        for k, v in d.items():
            agg[k] = max(agg.get(k, 0.0), v)

    for cid, n, F, r, w, c in cases.gram_cases():
        x, _, rows, wv, cv = cases.gram_inputs(n, F, r, w, c)
        record("gram", cid, F, {"colsum": cases.rel(cpu.colsum(x, rows, wv, cpu.F32), cpu.colsum(x, rows, wv)),
                                "gram": cases.rel(cpu.gram(x, rows, wv, cv, cpu.F32), cpu.gram(x, rows, wv, cv))})
    for cid, n, F, r, kind in cases.sweep_cases():
        x, y, rows, coef, icpt, cw = cases.sweep_inputs(n, F, r, kind)
        s32, s64 = (cpu.sweep(x, y, coef, icpt, cw, rows, dt) for dt in (cpu.F32, cpu.F64))
        if kind == "margin80":
            assert np.abs(s64["margins"]).max() >= 80 and np.isfinite(s32["loss"]), np.abs(s64["margins"]).max()
        d = {k: cases.rel(s32[k], s64[k]) for k in ("margins", "d", "grad", "curv")}
        d["loss"] = abs(s32["loss"] - s64["loss"]) / abs(s64["loss"])
        record("sweep", cid, F, d)
    for cid, n, F, r, lab in cases.project_cases():
        x, y, rows, W, c = cases.project_inputs(n, F, r, lab)
        (z32, cs32, _), (z64, cs64, _) = (cpu.project(x, W, c, y, rows, dt) for dt in (cpu.F32, cpu.F64))
        d = {"Z": cases.rel(z32, z64)}
        if lab:
            d["class_sums"] = cases.rel(cs32, cs64)
        record("project", cid, F, d)
    for n, F, seed in cases.E2E:
        x, y = cases.make_features(n, F, seed)
        ev = cases.assert_separated(x)
        r32, r64 = (cpu.run(x, y, cases.SPLIT_SEED, tol=tol, dt=dt) for dt, tol in ((cpu.F32, 1e-6), (cpu.F64, 1e-12)))
        assert r64["fit"]["converged"] and r32["fit"]["converged"], (r64["fit"], r32["fit"])
        assert r64["accuracy"] < 1.0, r64["accuracy"]
        d = {k: cases.rel(r32[k], r64[k]) for k in ("ratios", "components", "theta", "test_margins", "Z", "class_means")}
        excused = int((np.abs(r64["test_margins"]) < 100 * d["test_margins"] * np.abs(r64["test_margins"]).max()).sum())
        assert excused == 0, excused  # the seeds are chosen so that the oracle excuses no test row
        d.update({"min_abs_margin": float(np.abs(r64["test_margins"]).min()), "max_abs_margin": float(np.abs(r64["test_margins"]).max()),
                  "oracle_accuracy": r64["accuracy"], "oracle_iterations": r64["fit"]["iterations"],
                  "fp32_iterations": r32["fit"]["iterations"], "eigenvalues": [float(v) for v in cases.leading_eigenvalues(x)]})
        out["e2e"][cases.group_key(F)] = d
        print("e2e", (n, F), d, ev, flush=True)
        try:
            from sklearn.decomposition import PCA
            from sklearn.linear_model import LogisticRegression
        except ImportError:
            continue
        clf = LogisticRegression(class_weight="balanced", tol=1e-10, max_iter=10000).fit(x[r64["train"]].astype(np.float64), y[r64["train"]])
        p = PCA(n_components=2, svd_solver="full").fit(x.astype(np.float64))
        sk = {"theta": cases.rel(np.concatenate([clf.coef_[0], clf.intercept_]), r64["theta"]),
              "ratios": cases.rel(p.explained_variance_ratio_, r64["ratios"]), "components": cases.rel(p.components_, r64["components"])}
        out["sklearn"][cases.group_key(F)] = sk
        print("sklearn", (n, F), sk, flush=True)
    path = os.path.join(os.path.dirname(HERE), "golden", "validate_fp32_distances.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
