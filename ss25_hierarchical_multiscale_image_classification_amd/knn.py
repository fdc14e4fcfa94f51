"""The weighted k-nearest-neighbour probe of ``--validate --validate_knn K``: the ctypes binding of include/hipac_knn.h
(``csrc/knn.hip``) and the classifier over it.

The protocol is Wu et al. 2018's, the one SimCLR, MoCo and DINO report next to the linear probe: every test row votes with
its K most similar training rows, neighbour t weighing ``exp((s_t - s_0) / T)`` (relative to the best neighbour, so nothing
overflows).  The similarity is the cosine (``inv_norms`` gives the scales), computed in exact float32 on the device; the
[n_test, n_train] similarity matrix is never written, ``hipac_knn_topk`` keeps K numbers per test row.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import capi

KNN_ABI_VERSION = 1  # include/hipac_knn.h HIPAC_KNN_ABI_VERSION this binding was written against
MAX_K = 256          # HIPAC_KNN_MAX_K

# name -> (restype, argtypes); must list every symbol include/hipac_knn.h declares (tests/test_knn_capi_symbols.py)
KNN_SYMBOLS = {
    "hipac_knn_abi_version": (C.c_int, []),
    "hipac_knn_inv_norms": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_knn_bank_splits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hipac_knn_topk_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hipac_knn_topk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hipac_knn_vote": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
}

_bound = None


def load_knn_library():
    """The library of ``capi.load_library()`` with the k-NN entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, KNN_SYMBOLS, "hipac_knn_abi_version", KNN_ABI_VERSION, "knn ABI")
    return lib


def _rows(X: torch.Tensor, rows: Optional[torch.Tensor], name: str, check_rows: bool) -> int:
    """-> the number of rows the list (None = identity) selects, after the checks the library leaves to its caller."""
    if rows is None:
        return int(X.shape[0])
    if rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != X.device or rows.numel() == 0:
        raise capi.HipacError(f"{name} must be a non-empty int32[n] on the device of X")
    if check_rows and (int(rows.min()) < 0 or int(rows.max()) >= X.shape[0]):
        raise capi.HipacError(f"{name} must lie in 0..{X.shape[0] - 1}")
    return int(rows.numel())


def _matrix(X: torch.Tensor, *others):
    capi._require_gpu(X, *others)
    if X.dtype != torch.float32 or X.dim() != 2:
        raise capi.HipacError("X must be float32[n_feat_rows, F]")


def _vector(t: Optional[torch.Tensor], X: torch.Tensor, shape, name: str, dtype=torch.float32):
    if t is not None and (t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != X.device or not t.is_contiguous()):
        raise capi.HipacError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the device of X")
    return t


def inv_norms(X: torch.Tensor, rows: Optional[torch.Tensor] = None, check_rows: bool = True) -> torch.Tensor:
    """out[i] = 1 / max(|X[rows[i]]|, 1e-12), float32[n]."""
    _matrix(X, rows)
    n = _rows(X, rows, "rows", check_rows)
    out = torch.empty(n, dtype=torch.float32, device=X.device)
    lib = load_knn_library()
    with torch.cuda.device(X.device):
        rc = lib.hipac_knn_inv_norms(X.data_ptr(), int(X.shape[0]), capi._ptr(rows), n, int(X.shape[1]), out.data_ptr(), capi._stream())
    capi._check(rc, "hipac_knn_inv_norms")
    return out


def topk(X: torch.Tensor, k: int, q_rows: Optional[torch.Tensor] = None, b_rows: Optional[torch.Tensor] = None,
         q_scale: Optional[torch.Tensor] = None, b_scale: Optional[torch.Tensor] = None, check_rows: bool = True
         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """For every query row X[q_rows[i]] the k bank rows X[b_rows[j]] of largest (X[q] . X[b]) * q_scale[i] * b_scale[j]
    (a scale of None is 1).  -> (sim float32[n_q, k], idx int32[n_q, k]): bank POSITIONS j, descending similarity, equal
    similarities by ascending position, NaN after -inf."""
    _matrix(X, q_rows, b_rows, q_scale, b_scale)
    n_q, n_b = _rows(X, q_rows, "q_rows", check_rows), _rows(X, b_rows, "b_rows", check_rows)
    _vector(q_scale, X, (n_q,), "q_scale")
    _vector(b_scale, X, (n_b,), "b_scale")
    F, k = int(X.shape[1]), int(k)
    lib = load_knn_library()
    need = lib.hipac_knn_topk_workspace_bytes(n_q, n_b, F, k)
    if need == 0:
        raise capi.HipacError(f"k-NN search of {n_q} x {n_b} x {F}, k = {k} refused (1 <= n_q <= 2^24, 1 <= k <= {MAX_K}, "
                              "k <= n_b <= 2^24, F a multiple of 4 in 4..2048)")
    ws = torch.empty(need, dtype=torch.uint8, device=X.device)
    sim = torch.empty((n_q, k), dtype=torch.float32, device=X.device)
    idx = torch.empty((n_q, k), dtype=torch.int32, device=X.device)
    with torch.cuda.device(X.device):
        rc = lib.hipac_knn_topk(X.data_ptr(), int(X.shape[0]), F, capi._ptr(q_rows), n_q, capi._ptr(q_scale), capi._ptr(b_rows), n_b,
                                capi._ptr(b_scale), k, sim.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), capi._stream())
    capi._check(rc, "hipac_knn_topk")
    return sim, idx


def vote(sim: torch.Tensor, idx: torch.Tensor, bank_labels: torch.Tensor, temperature: float, class_w) -> Tuple[torch.Tensor, torch.Tensor]:
    """The weighted vote over the lists of ``topk``; bank_labels int32[n_b] (0 / 1, by bank position), class_w two weights.
    -> (scores float64[n_q, 2], pred int32[n_q]); a tie goes to class 0."""
    capi._require_gpu(sim, idx, bank_labels)
    if sim.dtype != torch.float32 or sim.dim() != 2 or idx.dtype != torch.int32 or idx.shape != sim.shape or idx.device != sim.device:
        raise capi.HipacError("sim must be float32[n_q, k] and idx int32[n_q, k] on one device")
    if bank_labels.dtype != torch.int32 or bank_labels.dim() != 1 or bank_labels.device != sim.device:
        raise capi.HipacError("bank_labels must be int32[n_b] on the device of sim")
    if not temperature > 0:
        raise capi.HipacError(f"temperature {temperature}: must be positive")
    n_q, k = int(sim.shape[0]), int(sim.shape[1])
    cw = torch.tensor([float(class_w[0]), float(class_w[1])], dtype=torch.float64, device=sim.device)
    scores = torch.empty((n_q, 2), dtype=torch.float64, device=sim.device)
    pred = torch.empty(n_q, dtype=torch.int32, device=sim.device)
    lib = load_knn_library()
    with torch.cuda.device(sim.device):
        rc = lib.hipac_knn_vote(sim.data_ptr(), idx.data_ptr(), bank_labels.data_ptr(), n_q, k, 1.0 / float(temperature), cw.data_ptr(),
                                scores.data_ptr(), pred.data_ptr(), capi._stream())
    capi._check(rc, "hipac_knn_vote")
    return scores, pred


def knn_classify(X: torch.Tensor, y: torch.Tensor, train_rows: torch.Tensor, test_rows: torch.Tensor, k: int, temperature: float,
                 class_w) -> Dict[str, torch.Tensor]:
    """Classify the rows ``test_rows`` of X by their k nearest (cosine) rows among ``train_rows``; y holds the labels
    (0 / 1) of all rows of X.  -> sim, idx (positions in train_rows), neighbours (row numbers of X, int32[n_test, k]),
    scores, pred; all on the device."""
    q_scale = inv_norms(X, test_rows)
    b_scale = inv_norms(X, train_rows, check_rows=True)
    sim, idx = topk(X, k, q_rows=test_rows, b_rows=train_rows, q_scale=q_scale, b_scale=b_scale, check_rows=False)
    bank_labels = y[train_rows.long()].to(torch.int32).contiguous()
    scores, pred = vote(sim, idx, bank_labels, temperature, class_w)
    neighbours = train_rows[idx.long()].contiguous()
    return {"sim": sim, "idx": idx, "neighbours": neighbours, "scores": scores, "pred": pred}
