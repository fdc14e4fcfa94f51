"""Gated attention pooling for the MIL head (``--mil_gated``): the ctypes binding of include/hipac_mil_gated.h
(``csrc/mil_gated.hip``).

The gated attention mechanism of Ilse et al. 2018 (ABMIL, eq. 9; the form CLAM and most CAMELYON16 MIL baselines use): the
score of a patch is ``attn_U(tanh(attn_V(x)) * sigmoid(attn_G(x)))`` with a third ``aggregator.attn_G = Linear(feature_dim,
attn_dim)``.  Everything after the hidden layer -- scores, per-head softmax, pooling, classifier -- is that of ``mil_heads.py``,
so the gate composes with ``--mil_heads K``.  The model is ``mil.MILClassifier(..., gated=True)``; a state_dict is gated if
it holds ``aggregator.attn_G.weight``.  This module holds what talks to the library:

* ``gated_forward``: ``hipac_mil_gated_forward`` -- many bags of contiguous rows scored in one call (inference).
* ``load_mil_gated_library``: the bound library; ``mil_train.NativeMILTrainer`` runs ``hipac_mil_gated_train_fwd_bwd``
  through it when its model is gated, for any head count.

An ungated model never comes here: ``mil.MILClassifier`` and ``mil_train.NativeMILTrainer`` keep sending it through the
entry points it always took.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import capi
from .mil_heads import MAX_HEADS

MIL_GATED_ABI_VERSION = 1  # include/hipac_mil_gated.h HIPAC_MIL_GATED_ABI_VERSION this binding was written against

GATE_W, GATE_B = "aggregator.attn_G.weight", "aggregator.attn_G.bias"


class MilGatedParams(C.Structure):  # hipac_mil_gated_params_t
    _fields_ = [("base", capi.MilParams), ("attn_G_w", C.c_void_p), ("attn_G_b", C.c_void_p)]


# name -> (restype, argtypes); must list every symbol include/hipac_mil_gated.h declares (tests/test_mil_gated_capi_symbols.py)
MIL_GATED_SYMBOLS = {
    "hipac_mil_gated_abi_version": (C.c_int, []),
    "hipac_mil_gated_forward_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_gated_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hipac_mil_gated_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_gated_train_fwd_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_int, C.c_void_p]),
}

_bound = None


def load_mil_gated_library():
    """The library of ``capi.load_library()`` with the gated entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, MIL_GATED_SYMBOLS, "hipac_mil_gated_abi_version", MIL_GATED_ABI_VERSION,
                                   "MIL gated ABI")
    return lib


def is_gated(sd: Dict[str, torch.Tensor]) -> bool:
    """Whether a MILClassifier state_dict is a gated model: it holds ``aggregator.attn_G.weight``."""
    return GATE_W in sd


def gated_dims(sd: Dict[str, torch.Tensor]) -> Tuple[int, int, int]:
    """(heads, feature_dim, attn_dim) of a gated MILClassifier state_dict; ValueError when a key is missing or the shapes
    of ``attn_V``, ``attn_G``, ``attn_U`` and the classifier do not agree.  Reads shapes only: nothing is launched."""
    keys = ("aggregator.attn_V.weight", "aggregator.attn_V.bias", "aggregator.attn_U.weight", "aggregator.attn_U.bias", GATE_W, GATE_B,
            "classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias")
    missing = [k for k in keys if k not in sd]
    if missing:
        raise ValueError(f"gated state_dict lacks {missing}")
    shape = {k: tuple(sd[k].shape) for k in keys}
    if len(shape["aggregator.attn_V.weight"]) != 2 or len(shape["aggregator.attn_U.weight"]) != 2:
        raise ValueError("aggregator.attn_V.weight and aggregator.attn_U.weight must be matrices")
    A, F = shape["aggregator.attn_V.weight"]
    K = shape["aggregator.attn_U.weight"][0]
    if not 1 <= K <= MAX_HEADS:
        raise ValueError(f"aggregator.attn_U.weight has {K} rows: 1..{MAX_HEADS} heads are supported")
    if shape["aggregator.attn_V.bias"] != (A,):
        raise ValueError("aggregator.attn_V.bias does not match aggregator.attn_V.weight")
    if shape[GATE_W] != (A, F) or shape[GATE_B] != (A,):
        raise ValueError(f"aggregator.attn_G must have the shapes of aggregator.attn_V ({A}, {F}) and ({A},), "
                         f"got {shape[GATE_W]} and {shape[GATE_B]}")
    if shape["aggregator.attn_U.weight"] != (K, A) or shape["aggregator.attn_U.bias"] != (K,):
        raise ValueError("aggregator.attn_U does not match aggregator.attn_V")
    hidden = shape["classifier.0.weight"][0]
    if shape["classifier.0.weight"] != (hidden, K * F) or shape["classifier.0.bias"] != (hidden,):
        raise ValueError(f"classifier.0.weight has {shape['classifier.0.weight'][-1]} columns, heads * feature_dim = {K} * {F} = {K * F}")
    classes = shape["classifier.2.weight"][0]
    if shape["classifier.2.weight"] != (classes, hidden) or shape["classifier.2.bias"] != (classes,):
        raise ValueError("classifier.2 does not match classifier.0.weight")
    return K, F, A


def mil_gated_params(sd: Dict[str, torch.Tensor], dev) -> Tuple[MilGatedParams, int]:
    """(hipac_mil_gated_params_t over the tensors of a gated MILClassifier state_dict, heads); ValueError on a shape that does
    not agree (``gated_dims``), HipacError on a tensor that is not contiguous float32 on ``dev``."""
    K, F, A = gated_dims(sd)
    w = lambda key: capi.mil_weight_ptr(sd, key, dev)
    g = MilGatedParams()
    p = g.base
    p.attn_V_w, p.attn_V_b = w("aggregator.attn_V.weight"), w("aggregator.attn_V.bias")
    p.attn_U_w, p.attn_U_b = w("aggregator.attn_U.weight"), w("aggregator.attn_U.bias")
    p.fc1_w, p.fc1_b = w("classifier.0.weight"), w("classifier.0.bias")
    p.fc2_w, p.fc2_b = w("classifier.2.weight"), w("classifier.2.bias")
    g.attn_G_w, g.attn_G_b = w(GATE_W), w(GATE_B)
    p.feature_dim, p.attn_dim, p.hidden_dim = F, A, int(sd["classifier.0.weight"].shape[0])
    p.num_classes = int(sd["classifier.2.weight"].shape[0])
    return g, K


def gated_forward(sd: Dict[str, torch.Tensor], feats: torch.Tensor, bag_offsets, want_attn: bool = True, want_pooled: bool = False
                  ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Score many bags at once with a gated K-head model.  ``sd``: MILClassifier state_dict tensors with the ``attn_G`` keys
    (float32, on the device of ``feats``); ``feats`` float32[n, F] with the rows of a bag contiguous; ``bag_offsets``
    int[n_bags + 1] (validated on the host).  -> (logits[n_bags, C], attn[n, K] or None, pooled[n_bags, K F] or None).
    The shapes are checked first (ValueError), before the library is loaded or anything is launched."""
    K, F, _ = gated_dims(sd)
    if not torch.is_tensor(feats) or feats.dim() != 2 or int(feats.shape[1]) != F:
        raise ValueError(f"feats must be float32[n, {F}] (the columns of aggregator.attn_V.weight)")
    capi._require_gpu(feats)
    if feats.dtype != torch.float32:
        raise capi.HipacError("feats must be float32[n, feature_dim]")
    n = int(feats.shape[0])
    offs_host, _ = capi.check_bag_offsets(bag_offsets, n)
    lib = load_mil_gated_library()
    g, K = mil_gated_params(sd, feats.device)
    return capi._mil_head_forward(lib, "hipac_mil_gated_forward", "hipac_mil_gated_forward_workspace_bytes", g, K, feats, offs_host, (),
                                  (n, K) if want_attn else None, K * F if want_pooled else 0, "gated")
