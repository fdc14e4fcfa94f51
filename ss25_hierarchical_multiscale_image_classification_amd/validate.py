"""The feature sanity check (``--validate``): the ctypes binding of include/hipac_validate.h (``csrc/validate.hip``)
and the driver over it.

The reference's ``validate_resnet_classifier`` (src/main.py:1017-1070) hands what ``--extract_features`` wrote to
scikit-learn: a two-component PCA, t-SNE, a stratified 80/20 split and ``LogisticRegression(class_weight="balanced")``.
Here the feature matrix goes to the device once and stays there:

* PCA: the column sums give the mean, ``hipac_validate_gram`` the centred scatter matrix; ``numpy.linalg.eigh`` of the
  F x F covariance runs on the host in float64 (1 MB at F = 512); ``hipac_validate_project`` projects the rows and adds
  the projections up per class.
* the probe: Newton's method on scikit-learn's objective.  ``hipac_validate_logistic_sweep`` gives loss, gradient and the
  curvature weights in one read of the training rows, ``hipac_validate_gram`` with those weights the Hessian; the
  (F + 1) x (F + 1) solve runs on the host in float64.  The training and the test rows are index lists into the one
  matrix.

* the k-NN probe (``knn_k`` > 0, knn.py): the weighted k-nearest-neighbour classifier of Wu et al. 2018 on the probe's split
  and under its class weights; the search runs on the device and keeps K numbers per test row.

Deliberately different from the reference: no t-SNE; our own split (``stratified_split``), not scikit-learn's shuffle;
Newton instead of L-BFGS (the objective is strictly convex: same optimum); eigen-decomposition of the covariance
instead of an SVD of the centred matrix; float32 sums on the device.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import capi
from .mil_train import classification_metrics

VALIDATE_ABI_VERSION = 1  # include/hipac_validate.h HIPAC_VALIDATE_ABI_VERSION this binding was written against
MAX_COMPONENTS = 4        # HIPAC_VALIDATE_MAX_COMPONENTS

_ROWS = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]  # X, n_feat_rows, rows, n, F
_WS = [C.c_void_p, C.c_size_t, C.c_void_p]                  # workspace, workspace_bytes, stream
# name -> (restype, argtypes); must list every symbol include/hipac_validate.h declares (tests/test_validate_capi_symbols.py)
VALIDATE_SYMBOLS = {
    "hipac_validate_abi_version": (C.c_int, []),
    "hipac_validate_colsum_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hipac_validate_colsum": (C.c_int, [*_ROWS, C.c_void_p, C.c_void_p, *_WS]),
    "hipac_validate_gram_slices": (C.c_int, [C.c_int, C.c_int]),
    "hipac_validate_gram_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hipac_validate_gram": (C.c_int, [*_ROWS, C.c_void_p, C.c_void_p, C.c_void_p, *_WS]),
    "hipac_validate_logistic_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hipac_validate_logistic_sweep": (C.c_int, [*_ROWS, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, *_WS]),
    "hipac_validate_project_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hipac_validate_project": (C.c_int, [*_ROWS, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         *_WS]),
}

_bound = None


def load_validate_library():
    """The library of ``capi.load_library()`` with the validate entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, VALIDATE_SYMBOLS, "hipac_validate_abi_version", VALIDATE_ABI_VERSION, "validate ABI")
    return lib


# ----------------------------------------------------------------------------
# the four entry points
# ----------------------------------------------------------------------------


def _matrix(X: torch.Tensor, rows: Optional[torch.Tensor], check_rows: bool) -> Tuple[int, int, int]:
    """-> (n_feat_rows, n, F) after the checks the library leaves to its caller."""
    capi._require_gpu(X, rows)
    if X.dtype != torch.float32 or X.dim() != 2:
        raise capi.HipacError("X must be float32[n_feat_rows, F]")
    if rows is None:
        return int(X.shape[0]), int(X.shape[0]), int(X.shape[1])
    if rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != X.device or rows.numel() == 0:
        raise capi.HipacError("rows must be a non-empty int32[n] on the device of X")
    if check_rows and (int(rows.min()) < 0 or int(rows.max()) >= X.shape[0]):
        raise capi.HipacError(f"rows must lie in 0..{X.shape[0] - 1}")
    return int(X.shape[0]), int(rows.numel()), int(X.shape[1])


def _vector(t: Optional[torch.Tensor], X: torch.Tensor, shape, name: str, dtype=torch.float32):
    if t is not None and (t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != X.device or not t.is_contiguous()):
        raise capi.HipacError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the device of X")
    return t


def _workspace(need: int, what: str, X: torch.Tensor) -> torch.Tensor:
    if need == 0:
        raise capi.HipacError(f"{what} refused (1 <= n <= 2^24, F a multiple of 4 in 4..2048)")
    return torch.empty(need, dtype=torch.uint8, device=X.device)


def colsum(X: torch.Tensor, rows: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None, check_rows: bool = True
           ) -> torch.Tensor:
    """out[F] = sum_i w[i] X[rows[i]] (w None = 1)."""
    nf, n, F = _matrix(X, rows, check_rows)
    _vector(w, X, (n,), "w")
    lib = load_validate_library()
    ws = _workspace(lib.hipac_validate_colsum_workspace_bytes(n, F), f"column sums of {n} x {F}", X)
    out = torch.empty(F, dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        rc = lib.hipac_validate_colsum(X.data_ptr(), nf, capi._ptr(rows), n, F, capi._ptr(w), out.data_ptr(), ws.data_ptr(),
                                       ws.numel(), capi._stream())
    capi._check(rc, "hipac_validate_colsum")
    return out


def gram(X: torch.Tensor, rows: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None, c: Optional[torch.Tensor] = None,
         check_rows: bool = True) -> torch.Tensor:
    """G[F, F] = sum_i w[i] (X[rows[i]] - c) (X[rows[i]] - c)^T (w None = 1, c None = 0); exactly symmetric."""
    nf, n, F = _matrix(X, rows, check_rows)
    _vector(w, X, (n,), "w")
    _vector(c, X, (F,), "c")
    lib = load_validate_library()
    ws = _workspace(lib.hipac_validate_gram_workspace_bytes(n, F), f"Gram matrix of {n} x {F}", X)
    G = torch.empty((F, F), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        rc = lib.hipac_validate_gram(X.data_ptr(), nf, capi._ptr(rows), n, F, capi._ptr(w), capi._ptr(c), G.data_ptr(), ws.data_ptr(),
                                     ws.numel(), capi._stream())
    capi._check(rc, "hipac_validate_gram")
    return G


def logistic_sweep(X: torch.Tensor, labels: torch.Tensor, coef: torch.Tensor, intercept: torch.Tensor, class_w: torch.Tensor,
                   rows: Optional[torch.Tensor] = None, want_margins: bool = False, check_rows: bool = True
                   ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """One sweep of the probe over the rows ``rows`` of X (labels int64[n_feat_rows], 0 / 1, read through ``rows``).
    -> (sums[2 F + 3] = sum r x | sum d x | sum r | sum d | loss sum, d[n], margins[n] or None)."""
    nf, n, F = _matrix(X, rows, check_rows)
    _vector(labels, X, (nf,), "labels", torch.int64)
    _vector(coef, X, (F,), "coef")
    _vector(intercept, X, (1,), "intercept")
    _vector(class_w, X, (2,), "class_w")
    lib = load_validate_library()
    ws = _workspace(lib.hipac_validate_logistic_workspace_bytes(n, F), f"logistic sweep of {n} x {F}", X)
    sums = torch.empty(2 * F + 3, dtype=torch.float32, device=X.device)
    d = torch.empty(n, dtype=torch.float32, device=X.device)
    margins = torch.empty(n, dtype=torch.float32, device=X.device) if want_margins else None
    with torch.cuda.device(X.device):
        rc = lib.hipac_validate_logistic_sweep(X.data_ptr(), nf, capi._ptr(rows), n, F, coef.data_ptr(), intercept.data_ptr(),
                                               labels.data_ptr(), class_w.data_ptr(), sums.data_ptr(), d.data_ptr(),
                                               capi._ptr(margins), ws.data_ptr(), ws.numel(), capi._stream())
    capi._check(rc, "hipac_validate_logistic_sweep")
    return sums, d, margins


def project(X: torch.Tensor, W: torch.Tensor, c: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
            rows: Optional[torch.Tensor] = None, check_rows: bool = True
            ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Z[n, K] = (X[rows[i]] - c) . W[k], K <= 4.  With labels (int64[n_feat_rows], 0 / 1): also the sums of Z per class
    [2, K] and the rows per class [2] (float32, exact)."""
    nf, n, F = _matrix(X, rows, check_rows)
    if W.dim() != 2 or not 1 <= W.shape[0] <= MAX_COMPONENTS:
        raise capi.HipacError(f"W must be float32[K, F] with K in 1..{MAX_COMPONENTS}")
    K = int(W.shape[0])
    _vector(W, X, (K, F), "W")
    _vector(c, X, (F,), "c")
    _vector(labels, X, (nf,), "labels", torch.int64)
    lib = load_validate_library()
    ws = _workspace(lib.hipac_validate_project_workspace_bytes(n, F, K), f"projection of {n} x {F}", X)
    Z = torch.empty((n, K), dtype=torch.float32, device=X.device)
    sums = torch.empty((2, K), dtype=torch.float32, device=X.device) if labels is not None else None
    counts = torch.empty(2, dtype=torch.float32, device=X.device) if labels is not None else None
    with torch.cuda.device(X.device):
        rc = lib.hipac_validate_project(X.data_ptr(), nf, capi._ptr(rows), n, F, capi._ptr(c), W.data_ptr(), K, capi._ptr(labels),
                                        Z.data_ptr(), capi._ptr(sums), capi._ptr(counts), ws.data_ptr(), ws.numel(), capi._stream())
    capi._check(rc, "hipac_validate_project")
    return Z, sums, counts


# ----------------------------------------------------------------------------
# host pieces
# ----------------------------------------------------------------------------


def check_labels(labels) -> np.ndarray:
    """-> labels as int64[N]; ValueError unless every one is 0 or 1."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.dtype.kind not in "iub" or (lab.size and (lab.min() < 0 or lab.max() > 1)):
        raise ValueError("the labels must be a vector of 0 (normal) and 1 (tumor)")
    return lab.astype(np.int64)


def stratified_split(labels, seed: int, test_fraction: float = 0.2) -> Tuple[np.ndarray, np.ndarray]:
    """(train rows, test rows), both ascending.  One ``Generator(PCG64(seed))``; for class 0 then class 1 it permutes the
    class's row numbers, and the first max(1, floor(test_fraction n_c + 0.5)) of the permutation are test rows.
    ValueError unless both classes have at least two rows."""
    lab = np.asarray(labels)
    rng = np.random.Generator(np.random.PCG64(seed))
    train, test = [], []
    for cls in (0, 1):
        idx = np.flatnonzero(lab == cls)
        if idx.size < 2:
            raise ValueError(f"class {cls} has {idx.size} row(s): the split needs at least 2 of each class")
        perm = rng.permutation(idx)
        k = max(1, int(np.floor(test_fraction * idx.size + 0.5)))
        test.append(perm[:k])
        train.append(perm[k:])
    return np.sort(np.concatenate(train)).astype(np.int64), np.sort(np.concatenate(test)).astype(np.int64)


def flip_signs(components: np.ndarray) -> np.ndarray:
    """Each row times +-1 so that its entry of largest magnitude is positive (scikit-learn >= 1.5's svd_flip on V)."""
    comp = np.array(components, copy=True)
    big = np.argmax(np.abs(comp), axis=1)
    sign = np.sign(comp[np.arange(comp.shape[0]), big])
    sign[sign == 0] = 1
    return comp * sign[:, None]


def top_components(cov: np.ndarray, k: int = 2) -> Tuple[np.ndarray, np.ndarray]:
    """(explained-variance ratios [k], components [k, F], sign-fixed) of a covariance matrix, in float64."""
    evals, evecs = np.linalg.eigh(np.asarray(cov, np.float64))
    order = np.argsort(evals)[::-1][:k]
    total = float(np.trace(cov))
    ratios = evals[order] / total if total > 0 else np.zeros(len(order))
    return ratios, flip_signs(evecs[:, order].T)


def balanced_class_weights(train_labels) -> np.ndarray:
    """scikit-learn's class_weight="balanced": n / (2 n_c)."""
    t = np.asarray(train_labels)
    return t.size / (2.0 * np.array([(t == 0).sum(), (t == 1).sum()], np.float64))


# ----------------------------------------------------------------------------
# the driver
# ----------------------------------------------------------------------------


def pca_device(X: torch.Tensor, labels: Optional[torch.Tensor], k: int = 2) -> Dict[str, object]:
    """Two-component PCA of the rows of X on the device.  -> explained_variance_ratio [k], components float64 [k, F],
    mean float64 [F], projection (device, float32 [N, k]) and, with labels, class_means [2, k] (NaN for an absent class)."""
    N, F = int(X.shape[0]), int(X.shape[1])
    mean = colsum(X).cpu().numpy().astype(np.float64) / N
    c = torch.from_numpy(mean.astype(np.float32)).to(X.device)
    cov = gram(X, c=c).cpu().numpy().astype(np.float64) / max(N - 1, 1)
    ratios, comps = top_components(cov, k)
    W = torch.from_numpy(np.ascontiguousarray(comps, dtype=np.float32)).to(X.device)
    Z, sums, counts = project(X, W, c=c, labels=labels)
    out = {"explained_variance_ratio": ratios, "components": comps, "mean": mean, "projection": Z}
    if labels is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["class_means"] = sums.cpu().numpy().astype(np.float64) / counts.cpu().numpy().astype(np.float64)[:, None]
    return out


# A step is kept unless the loss rises by more than 8 eps |J|, eps that of the precision the loss sum is formed in (float32
# here): below that a rise is the sum's own rounding, not the step's doing.
LOSS_SLACK = 8 * float(np.finfo(np.float32).eps)


def fit_probe(X: torch.Tensor, labels: torch.Tensor, train_rows: torch.Tensor, class_w: np.ndarray, C_reg: float = 1.0,
              tol: float = 1e-4, max_iter: int = 100) -> Dict[str, object]:
    """Newton's method on J(w, b) = (1 / S) sum_i s_i l_i + |w|^2 / (2 C S) over the rows ``train_rows`` of X
    (S = sum_i s_i, s_i = class_w[y_i], the intercept unpenalised): scikit-learn's objective.  The step is halved while
    the loss does not decrease (a rise within ``LOSS_SLACK`` of |J| counts as none); stops at max |grad J| <= tol or after max_iter iterations.
    -> coef float32 [F], intercept float, iterations, gradient_norm, converged, loss."""
    F, dev = int(X.shape[1]), X.device
    n0 = int((labels[train_rows.long()] == 0).sum())
    S = float(class_w[0] * n0 + class_w[1] * (train_rows.numel() - n0))
    s_dev = torch.tensor(class_w, dtype=torch.float32, device=dev)
    reg = 1.0 / (C_reg * S)

    def evaluate(theta):
        coef = torch.from_numpy(theta[:F].copy()).to(dev)
        icpt = torch.from_numpy(theta[F:].copy()).to(dev)
        sums, d, _ = logistic_sweep(X, labels, coef, icpt, s_dev, rows=train_rows, check_rows=False)
        h = sums.cpu().numpy().astype(np.float64)
        w64 = theta[:F].astype(np.float64)
        J = h[2 * F + 2] / S + 0.5 * reg * float(w64 @ w64)
        g = np.concatenate([h[:F] / S + reg * w64, [h[2 * F] / S]])
        return J, g, h, d

    theta = np.zeros(F + 1, np.float32)
    J, g, h, d = evaluate(theta)
    iterations, converged = 0, False
    while True:
        gnorm = float(np.max(np.abs(g)))
        if gnorm <= tol:
            converged = True
            break
        if iterations >= max_iter:
            break
        H = np.empty((F + 1, F + 1), np.float64)
        H[:F, :F] = gram(X, rows=train_rows, w=d, check_rows=False).cpu().numpy().astype(np.float64) / S
        H[:F, :F] += reg * np.eye(F)
        H[:F, F] = H[F, :F] = h[F:2 * F] / S
        H[F, F] = h[2 * F + 1] / S
        try:
            delta = np.linalg.solve(H, -g)
        except np.linalg.LinAlgError:
            break
        t, accepted = 1.0, False
        for _ in range(30):
            trial = (theta.astype(np.float64) + t * delta).astype(np.float32)
            J2, g2, h2, d2 = evaluate(trial)
            if np.isfinite(J2) and J2 <= J + LOSS_SLACK * abs(J):
                theta, J, g, h, d, accepted = trial, J2, g2, h2, d2, True
                break
            t *= 0.5
        iterations += 1
        if not accepted:
            break
    return {"coef": theta[:F].copy(), "intercept": float(theta[F]), "iterations": iterations,
            "gradient_norm": float(np.max(np.abs(g))), "converged": converged, "loss": float(J)}


def knn_probe(X: torch.Tensor, y: torch.Tensor, lab: np.ndarray, train: np.ndarray, test: np.ndarray, train_rows: torch.Tensor,
              test_rows: torch.Tensor, class_w: np.ndarray, k: int, temperature: float) -> Dict[str, object]:
    """The weighted k-NN classifier (knn.py) on the probe's split, under the probe's class weights.  -> k, temperature,
    n_train, n_test, the metrics of ``classification_metrics`` on the test rows and ``neighbours`` int32 [n_test, 1 + k]: a
    test row number, then the row numbers of its neighbours, nearest first."""
    from . import knn

    r = knn.knn_classify(X, y, train_rows, test_rows, k, temperature, class_w)
    out: Dict[str, object] = {"k": int(k), "temperature": float(temperature), "n_train": int(train.size), "n_test": int(test.size)}
    out.update(classification_metrics(lab[test], r["pred"].cpu().numpy().astype(np.int64)))
    out["neighbours"] = np.concatenate([test.astype(np.int32)[:, None], r["neighbours"].cpu().numpy()], axis=1)
    return out


def run(features, labels, seed: int = 42, C_reg: float = 1.0, tol: float = 1e-4, max_iter: int = 100, device=None, knn_k: int = 0,
        knn_temperature: float = 0.07) -> Dict[str, object]:
    """The whole check on ``features`` float32 [N, F] and ``labels`` (0 / 1) [N].  -> a dict with the PCA
    (explained_variance_ratio, pca_class_means, components, projection as a float32 numpy array) and, when both classes
    have at least two rows, the probe (n_train, n_test, the metrics of ``classification_metrics`` on the test rows,
    newton_iterations, gradient_norm, converged, coef, intercept, test_rows, test_margins); otherwise ``probe_skipped``
    holds the reason.  With ``knn_k`` > 0 and the probe's split, ``knn`` holds the result of ``knn_probe``, or
    ``knn_skipped`` the reason why not."""
    lab = check_labels(labels)
    feats = np.ascontiguousarray(features, dtype=np.float32)
    if feats.ndim != 2 or feats.shape[0] != lab.shape[0] or feats.shape[0] == 0:
        raise ValueError(f"features {feats.shape} and labels {lab.shape} do not agree")
    dev = torch.device("cuda" if device is None else device)
    X = torch.from_numpy(feats).to(dev)
    y = torch.from_numpy(lab).to(dev)
    p = pca_device(X, y)
    out: Dict[str, object] = {
        "n": int(feats.shape[0]), "feature_dim": int(feats.shape[1]), "label_counts": [int((lab == 0).sum()), int((lab == 1).sum())],
        "explained_variance_ratio": [float(v) for v in p["explained_variance_ratio"]],
        "pca_class_means": [[float(v) for v in row] for row in p["class_means"]],
        "components": p["components"], "projection": p["projection"].cpu().numpy(),
    }
    try:
        train, test = stratified_split(lab, seed)
    except ValueError as e:
        out["probe_skipped"] = str(e)
        if knn_k > 0:
            out["knn_skipped"] = str(e)
        return out
    train_rows = torch.from_numpy(train.astype(np.int32)).to(dev)
    test_rows = torch.from_numpy(test.astype(np.int32)).to(dev)
    class_w = balanced_class_weights(lab[train])
    fit = fit_probe(X, y, train_rows, class_w, C_reg, tol, max_iter)
    coef = torch.from_numpy(fit["coef"]).to(dev)
    icpt = torch.tensor([fit["intercept"]], dtype=torch.float32, device=dev)
    _, _, margins = logistic_sweep(X, y, coef, icpt, torch.tensor(class_w, dtype=torch.float32, device=dev), rows=test_rows,
                                   want_margins=True, check_rows=False)
    margins = margins.cpu().numpy()
    out.update(classification_metrics(lab[test], (margins > 0).astype(np.int64)))
    out.update({"n_train": int(train.size), "n_test": int(test.size), "newton_iterations": fit["iterations"],
                "gradient_norm": fit["gradient_norm"], "converged": bool(fit["converged"]), "coef": fit["coef"],
                "intercept": fit["intercept"], "test_rows": test, "test_margins": margins})
    if knn_k > 0:
        if train.size < knn_k:
            out["knn_skipped"] = f"{train.size} training row(s): k = {knn_k} needs at least as many"
        else:
            out["knn"] = knn_probe(X, y, lab, train, test, train_rows, test_rows, class_w, knn_k, knn_temperature)
    return out


JSON_KEYS = ("explained_variance_ratio", "pca_class_means", "n_train", "n_test", "accuracy", "precision", "recall", "f1_score",
             "confusion_matrix", "newton_iterations", "gradient_norm", "converged")


def report(res: Dict[str, object]) -> Dict[str, object]:
    """Print the reference's lines for one result of ``run`` and return what goes into results/validate_<L>.json."""
    print(f"[INFO] PCA explained variance ratio (2 components): {np.asarray(res['explained_variance_ratio'])}")
    for cls in (0, 1):
        print(f"[INFO] PCA mean for class {cls}: {np.asarray(res['pca_class_means'][cls])}")
    print("[INFO] t-SNE: not computed (README, 'Feature sanity check').")
    if "probe_skipped" in res:
        print(f"[INFO] Logistic regression probe skipped: {res['probe_skipped']}.")
    else:
        cm = res["confusion_matrix"]
        print(f"[INFO] Logistic Regression Accuracy: {res['accuracy']:.4f}")
        print("[INFO] Confusion Matrix:")
        print(np.array([[cm["TN"], cm["FP"]], [cm["FN"], cm["TP"]]]))
    if "knn" in res:
        kn = res["knn"]
        cm = kn["confusion_matrix"]
        print(f"[INFO] k-NN (k = {kn['k']}, T = {kn['temperature']:g}) accuracy: {kn['accuracy']:.4f}")
        print("[INFO] k-NN Confusion Matrix:")
        print(np.array([[cm["TN"], cm["FP"]], [cm["FN"], cm["TP"]]]))
    elif "knn_skipped" in res:
        print(f"[INFO] k-NN probe skipped: {res['knn_skipped']}.")
    doc = {k: res[k] for k in JSON_KEYS if k in res}
    # an absent class has no mean: null in the file, not NaN
    doc["pca_class_means"] = [[None if v != v else v for v in row] for row in doc["pca_class_means"]]
    if "probe_skipped" in res:
        doc["probe_skipped"] = res["probe_skipped"]
    if "knn" in res:
        doc["knn"] = {k: v for k, v in res["knn"].items() if k != "neighbours"}
    elif "knn_skipped" in res:
        doc["knn_skipped"] = res["knn_skipped"]
    return doc
