"""The oracle of the --validate tests: a restatement of every quantity the device computes, on the CPU, independent of the
package under test.  The sums run in torch at the precision ``dt`` -- float64 is the oracle, float32 is what
tests/tools/measure_validate_fp32.py records as the distance float32 arithmetic itself keeps from it -- and the small dense
algebra (the F x F eigen-decomposition, the (F + 1) x (F + 1) Newton solve, the split) in numpy float64 either way, as in
the driver.  Inputs and outputs are numpy arrays.

Both reported quantities are defined without an algorithm: the leading eigenpairs of the covariance matrix (up to the sign
rule of ``flip_signs``) and the minimiser of the strictly convex
    J(w, b) = (1 / S) sum_i s_i (log(1 + exp(m_i)) - y_i m_i) + |w|^2 / (2 C S),   m_i = x_i . w + b,  S = sum_i s_i,
scikit-learn's objective for LogisticRegression(class_weight="balanced") with s_i = n / (2 n_{y_i}).
"""
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def _rows(x, rows, dt):
    xr = _t(x, dt)
    return xr if rows is None else xr[torch.from_numpy(np.asarray(rows, np.int64))]


def colsum(x, rows=None, w=None, dt=F64):
    xr = _rows(x, rows, dt)
    return (xr.sum(0) if w is None else (_t(w, dt)[:, None] * xr).sum(0)).numpy()


def gram(x, rows=None, w=None, c=None, dt=F64):
    xc = _rows(x, rows, dt)
    if c is not None:
        xc = xc - _t(c, dt)
    return (xc.T @ (xc if w is None else _t(w, dt)[:, None] * xc)).numpy()


def sweep(x, labels, coef, intercept, class_w, rows=None, dt=F64):
    """-> margins [n], d [n], loss (the sum), grad [F + 1] = sum r x | sum r, curv [F + 1] = sum d x | sum d."""
    xr = _rows(x, rows, dt)
    lab = np.asarray(labels) if rows is None else np.asarray(labels)[np.asarray(rows, np.int64)]
    y = _t(lab, dt)
    s = _t(np.asarray(class_w), dt)[torch.from_numpy(lab.astype(np.int64))]
    m = xr @ _t(coef, dt) + _t(intercept, dt)[0]
    e = torch.exp(-m.abs())
    p = torch.where(m >= 0, 1 / (1 + e), e / (1 + e))
    loss = (s * (m.clamp(min=0) + torch.log1p(e) - y * m)).sum()
    r, d = s * (p - y), s * (e / ((1 + e) * (1 + e)))
    return {"margins": m.numpy(), "d": d.numpy(), "loss": float(loss),
            "grad": torch.cat([r @ xr, r.sum()[None]]).numpy(), "curv": torch.cat([d @ xr, d.sum()[None]]).numpy()}


def project(x, W, c=None, labels=None, rows=None, dt=F64):
    """-> (Z [n, K], class sums [2, K] or None, class counts [2] or None)."""
    xr = _rows(x, rows, dt)
    if c is not None:
        xr = xr - _t(c, dt)
    Z = xr @ _t(W, dt).T
    if labels is None:
        return Z.numpy(), None, None
    lab = np.asarray(labels) if rows is None else np.asarray(labels)[np.asarray(rows, np.int64)]
    sums = torch.stack([Z[torch.from_numpy(lab == cls)].sum(0) for cls in (0, 1)])
    return Z.numpy(), sums.numpy(), np.array([(lab == 0).sum(), (lab == 1).sum()], np.float64)


def flip_signs(components):
    """Each row times +-1 so that its entry of largest magnitude is positive (scikit-learn >= 1.5)."""
    comp = np.array(components, np.float64)
    for row in comp:
        if row[np.argmax(np.abs(row))] < 0:
            row *= -1
    return comp


def pca(x, labels=None, k=2, dt=F64):
    """-> ratios [k], components [k, F], Z [N, k], class means [2, k] (None without labels)."""
    N = x.shape[0]
    mean = colsum(x, dt=dt).astype(np.float64) / N
    c = mean.astype(np.float32)  # the centre the device is handed
    cov = gram(x, c=c, dt=dt).astype(np.float64) / max(N - 1, 1)
    evals, evecs = np.linalg.eigh(cov)
    order = np.argsort(evals)[::-1][:k]
    comps = flip_signs(evecs[:, order].T)
    Z, sums, counts = project(x, comps.astype(np.float32), c=c, labels=labels, dt=dt)
    means = None if labels is None else sums.astype(np.float64) / counts[:, None]
    return evals[order] / np.trace(cov), comps, Z, means


def split(labels, seed, test_fraction=0.2):
    """The split rule: one Generator(PCG64(seed)); class 0 then class 1: permute the class's row numbers, the first
    max(1, floor(test_fraction n_c + 0.5)) are test rows; both lists ascending."""
    lab = np.asarray(labels)
    rng = np.random.Generator(np.random.PCG64(seed))
    train, test = [], []
    for cls in (0, 1):
        perm = rng.permutation(np.flatnonzero(lab == cls))
        k = max(1, int(np.floor(test_fraction * perm.size + 0.5)))
        test += list(perm[:k])
        train += list(perm[k:])
    return np.array(sorted(train), np.int64), np.array(sorted(test), np.int64)


def balanced_weights(train_labels):
    t = np.asarray(train_labels)
    return t.size / (2.0 * np.array([(t == 0).sum(), (t == 1).sum()], np.float64))


def newton(x, labels, train_rows, class_w, C=1.0, tol=1e-12, max_iter=100, dt=F64):
    """Newton's method on J over the rows ``train_rows``; the step is halved while the loss does not decrease (by more
    than the rounding of the loss sum, 8 eps |J| with the eps of ``dt``: the driver's rule).
    -> coef [F], intercept, iterations, gradient norm, converged."""
    F = x.shape[1]
    npdt = np.float64 if dt == F64 else np.float32
    lab = np.asarray(labels)[train_rows]
    S = float(class_w[0] * (lab == 0).sum() + class_w[1] * (lab == 1).sum())
    reg = 1.0 / (C * S)
    slack = 8 * float(np.finfo(npdt).eps)
    cw = np.asarray(class_w, npdt)

    def evaluate(theta):
        sw = sweep(x, labels, theta[:F], theta[F:], cw, rows=train_rows, dt=dt)
        w64 = theta[:F].astype(np.float64)
        J = sw["loss"] / S + 0.5 * reg * float(w64 @ w64)
        g = sw["grad"].astype(np.float64) / S
        g[:F] += reg * w64
        return J, g, sw

    theta = np.zeros(F + 1, npdt)
    J, g, sw = evaluate(theta)
    it, converged = 0, False
    while True:
        if np.max(np.abs(g)) <= tol:
            converged = True
            break
        if it >= max_iter:
            break
        H = np.empty((F + 1, F + 1), np.float64)
        H[:F, :F] = gram(x, rows=train_rows, w=sw["d"], dt=dt).astype(np.float64) / S + reg * np.eye(F)
        H[:F, F] = H[F, :F] = sw["curv"][:F].astype(np.float64) / S
        H[F, F] = float(sw["curv"][F]) / S
        delta = np.linalg.solve(H, -g)
        t, ok = 1.0, False
        for _ in range(30):
            trial = (theta.astype(np.float64) + t * delta).astype(npdt)
            J2, g2, sw2 = evaluate(trial)
            if np.isfinite(J2) and J2 <= J + slack * abs(J):
                theta, J, g, sw, ok = trial, J2, g2, sw2, True
                break
            t *= 0.5
        it += 1
        if not ok:
            break
    return {"coef": theta[:F].astype(np.float64), "intercept": float(theta[F]), "iterations": it,
            "gradient_norm": float(np.max(np.abs(g))), "converged": converged}


def run(x, labels, seed, C=1.0, tol=1e-12, dt=F64):
    """The whole check: PCA, split, probe, test margins and predictions."""
    ratios, comps, Z, means = pca(x, labels, dt=dt)
    train, test = split(labels, seed)
    cw = balanced_weights(np.asarray(labels)[train])
    fit = newton(x, labels, train, cw, C=C, tol=tol, dt=dt)
    npdt = np.float64 if dt == F64 else np.float32  # the margins at the run's own precision, as the device forms them
    margins = sweep(x, labels, fit["coef"].astype(npdt), np.array([fit["intercept"]], npdt), cw.astype(npdt), rows=test, dt=dt)["margins"]
    pred = (margins > 0).astype(np.int64)
    return {"ratios": ratios, "components": comps, "Z": Z, "class_means": means, "train": train, "test": test, "class_w": cw,
            "fit": fit, "theta": np.concatenate([fit["coef"], [fit["intercept"]]]), "test_margins": margins, "pred": pred,
            "accuracy": float((pred == np.asarray(labels)[test]).mean())}
