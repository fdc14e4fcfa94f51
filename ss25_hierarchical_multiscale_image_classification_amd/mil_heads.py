"""Multi-head attention pooling for the MIL head (``--mil_heads K``): the ctypes binding of include/hipac_mil_heads.h
(``csrc/mil_heads.hip``).

``experiments/experiment_configs.yaml`` asks for ``pooling: attention_heads: 8``: K attention branches over one shared
hidden layer (``ATTENTION_BRANCHES`` of Ilse et al.'s ABMIL).  ``aggregator.attn_U`` becomes ``Linear(attn_dim, K)``, the
softmax runs per head over the bag, the K pooled vectors are concatenated head-major and ``classifier.0`` becomes
``Linear(K * feature_dim, hidden)``; the state_dict keys stay.  The model is ``mil.MILClassifier(..., heads=K)``; this
module holds what talks to the library:

* ``heads_forward``: ``hipac_mil_heads_forward`` -- many bags of contiguous rows scored in one call (inference).
* ``load_mil_heads_library``: the bound library; ``mil_train.NativeMILTrainer`` runs ``hipac_mil_heads_train_fwd_bwd``
  through it when its model has more than one head.

K = 1 is the single-head model; ``mil.MILClassifier`` and ``mil_train.NativeMILTrainer`` keep sending it through
``hipac_mil_forward`` / ``hipac_mil_train_fwd_bwd``, so nothing an existing command line computes changes.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import capi

MIL_HEADS_ABI_VERSION = 1  # include/hipac_mil_heads.h HIPAC_MIL_HEADS_ABI_VERSION this binding was written against
MAX_HEADS = 8              # HIPAC_MIL_MAX_HEADS

# name -> (restype, argtypes); must list every symbol include/hipac_mil_heads.h declares (tests/test_mil_heads_capi_symbols.py)
MIL_HEADS_SYMBOLS = {
    "hipac_mil_heads_abi_version": (C.c_int, []),
    "hipac_mil_heads_forward_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_heads_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hipac_mil_heads_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_heads_train_fwd_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_int, C.c_void_p]),
}

_bound = None


def load_mil_heads_library():
    """The library of ``capi.load_library()`` with the multi-head entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, MIL_HEADS_SYMBOLS, "hipac_mil_heads_abi_version", MIL_HEADS_ABI_VERSION,
                                   "MIL heads ABI")
    return lib


def check_heads(heads) -> int:
    """-> heads as an int in 1..MAX_HEADS; ValueError otherwise."""
    if isinstance(heads, bool) or int(heads) != heads or not 1 <= int(heads) <= MAX_HEADS:
        raise ValueError(f"heads must be an integer in 1..{MAX_HEADS}, got {heads!r}")
    return int(heads)


def heads_of(sd: Dict[str, torch.Tensor]) -> int:
    """The head count of a MILClassifier state_dict: the rows of ``aggregator.attn_U.weight`` (1 without an aggregator)."""
    w = sd.get("aggregator.attn_U.weight")
    return 1 if w is None else int(w.shape[0])


def model_dims(sd: Dict[str, torch.Tensor], pooling: str) -> Tuple[int, int]:
    """(heads, feature_dim) of a MILClassifier state_dict; ValueError when ``classifier.0.weight`` does not have
    heads * feature_dim columns or the head count is outside 1..MAX_HEADS.  Mean / max pooling: (1, the columns)."""
    cols = int(sd["classifier.0.weight"].shape[1])
    if pooling != "attention":
        return 1, cols
    K, F = heads_of(sd), int(sd["aggregator.attn_V.weight"].shape[1])
    if not 1 <= K <= MAX_HEADS:
        raise ValueError(f"aggregator.attn_U.weight has {K} rows: 1..{MAX_HEADS} heads are supported")
    if cols != K * F:
        raise ValueError(f"classifier.0.weight has {cols} columns, heads * feature_dim = {K} * {F} = {K * F}")
    return K, F


def mil_heads_params(sd: Dict[str, torch.Tensor], F: int, dev) -> Tuple[capi.MilParams, int]:
    """(hipac_mil_params_t over the tensors of a multi-head MILClassifier state_dict, heads); the tensors must be contiguous
    float32 on ``dev`` and agree in shape: attn_U [K][A], classifier.0 [hidden][K F]."""
    w = lambda key: capi.mil_weight_ptr(sd, key, dev)
    p = capi.MilParams()
    p.attn_V_w, p.attn_V_b = w("aggregator.attn_V.weight"), w("aggregator.attn_V.bias")
    p.attn_U_w, p.attn_U_b = w("aggregator.attn_U.weight"), w("aggregator.attn_U.bias")
    p.fc1_w, p.fc1_b = w("classifier.0.weight"), w("classifier.0.bias")
    p.fc2_w, p.fc2_b = w("classifier.2.weight"), w("classifier.2.bias")
    A, K = int(sd["aggregator.attn_V.weight"].shape[0]), heads_of(sd)
    p.feature_dim, p.attn_dim, p.hidden_dim = F, A, int(sd["classifier.0.weight"].shape[0])
    p.num_classes = int(sd["classifier.2.weight"].shape[0])
    if not 1 <= K <= MAX_HEADS:
        raise capi.HipacError(f"aggregator.attn_U.weight has {K} rows: 1..{MAX_HEADS} heads are supported")
    if tuple(sd["aggregator.attn_V.weight"].shape) != (A, F):
        raise capi.HipacError("aggregator.attn_V.weight does not match feature_dim")
    if tuple(sd["aggregator.attn_U.weight"].shape) != (K, A) or tuple(sd["aggregator.attn_U.bias"].shape) != (K,):
        raise capi.HipacError("aggregator.attn_U does not match aggregator.attn_V")
    if tuple(sd["classifier.0.weight"].shape) != (p.hidden_dim, K * F):
        raise capi.HipacError(f"classifier.0.weight does not match heads * feature_dim = {K} * {F}")
    if tuple(sd["classifier.2.weight"].shape) != (p.num_classes, p.hidden_dim):
        raise capi.HipacError("classifier.2.weight does not match classifier.0.weight")
    return p, K


def heads_forward(sd: Dict[str, torch.Tensor], feats: torch.Tensor, bag_offsets, want_attn: bool = True, want_pooled: bool = False
                  ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Score many bags at once with a K-head model.  ``sd``: MILClassifier state_dict tensors (float32, on the device of
    ``feats``); ``feats`` float32[n, F] with the rows of a bag contiguous; ``bag_offsets`` int[n_bags + 1] (validated on the
    host).  -> (logits[n_bags, C], attn[n, K] or None, pooled[n_bags, K F] or None)."""
    capi._require_gpu(feats)
    if feats.dtype != torch.float32 or feats.dim() != 2:
        raise capi.HipacError("feats must be float32[n, feature_dim]")
    n, F = int(feats.shape[0]), int(feats.shape[1])
    offs_host, _ = capi.check_bag_offsets(bag_offsets, n)
    lib = load_mil_heads_library()
    p, K = mil_heads_params(sd, F, feats.device)
    return capi._mil_head_forward(lib, "hipac_mil_heads_forward", "hipac_mil_heads_forward_workspace_bytes", p, K, feats, offs_host, (),
                                  (n, K) if want_attn else None, K * F if want_pooled else 0, "multi-head")
