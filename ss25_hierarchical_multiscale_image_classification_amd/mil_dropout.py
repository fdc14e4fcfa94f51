"""Dropout and Monte-Carlo dropout uncertainty for the MIL head (include/hipac_mil_dropout.h, ``csrc/mil_dropout.hip``).

``experiments/experiment_configs.yaml`` asks for ``dropout_rate: 0.5`` and ``uncertainty_estimation: {method:
monte_carlo_dropout, num_samples: 100}``; the reference's ``src/utils/uncertainty.py`` holds ``monte_carlo_dropout`` (mean
and ``torch.var`` of the softmax outputs of ``num_samples`` stochastic forwards) and ``softmax_thresholding``, and its
``MILClassifier.uncertainty_estimation`` that was to call them is a TODO.

The mask is a counter-based one (Philox4x32-10, the header has the definition), so the device generates it where it reads
a feature row and the host can restate it: ``host_mask`` here is that restatement for the autograd path of
``mil.MILClassifier`` in ``train()`` mode; the device entry points are ``dropout_mask`` and ``mc_forward``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import capi

MIL_DROPOUT_ABI_VERSION = 1  # include/hipac_mil_dropout.h HIPAC_MIL_DROPOUT_ABI_VERSION this binding was written against
MC_MAX_SAMPLES = 4096

# name -> (restype, argtypes); must list every symbol include/hipac_mil_dropout.h declares (tests/test_mil_dropout_capi_symbols.py)
MIL_DROPOUT_SYMBOLS = {
    "hipac_mil_dropout_abi_version": (C.c_int, []),
    "hipac_mil_dropout_mask": (C.c_int, [C.c_double, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_mil_dropout_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_dropout_train_fwd_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_size_t, C.c_int, C.c_double, C.c_uint64, C.c_uint32, C.c_void_p]),
    "hipac_mil_mc_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_mc_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_uint64,
                                       C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

_bound = None


def load_mil_dropout_library():
    """The library of ``capi.load_library()`` with the dropout entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, MIL_DROPOUT_SYMBOLS, "hipac_mil_dropout_abi_version", MIL_DROPOUT_ABI_VERSION,
                                   "MIL dropout ABI")
    return lib


# ----------------------------------------------------------------------------
# the mask on the host
# ----------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _MASK32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 over arrays of counters (broadcast against each other) under one key -> four uint32 arrays."""
    c = [np.asarray(v, np.uint64) & np.uint64(_MASK32) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & _MASK32, int(k1) & _MASK32
    m32, s32 = np.uint64(_MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return [v.astype(np.uint32) for v in c]


def check_p(p: float) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise capi.HipacError(f"dropout probability must satisfy 0 <= p < 1, got {p}")
    return p


def threshold(p: float) -> int:
    """thr = floor(p * 2^32): an element is kept iff its word >= thr."""
    return int(np.floor(check_p(p) * 4294967296.0))


def scale(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - check_p(p)))


def host_mask(p: float, seed: int, sample: int, site: int, n_rows: int, n_cols: int, row0: int = 0) -> np.ndarray:
    """bool[n_rows, n_cols]: True where element (row0 + r, c) of (sample, site) is kept."""
    quads = (n_cols + 3) // 4
    rows = np.arange(row0, row0 + n_rows, dtype=np.uint64)[:, None]
    words = philox4x32_10(np.arange(quads, dtype=np.uint64)[None, :], rows, sample, site, seed & _MASK32, (seed >> 32) & _MASK32)
    flat = np.stack(words, axis=-1).reshape(n_rows, 4 * quads)[:, :n_cols]
    return flat >= np.uint32(threshold(p)) if threshold(p) else np.ones((n_rows, n_cols), bool)


def host_dropout(x: torch.Tensor, p: float, seed: int, sample: int, site: int, row0: int = 0) -> torch.Tensor:
    """x[n_rows, n_cols] (or [n_cols] = one row, row0) under the mask: kept elements times fl32 scale, the others 0;
    differentiable in x."""
    two_d = x if x.dim() == 2 else x.unsqueeze(0)
    keep = torch.from_numpy(host_mask(p, seed, sample, site, two_d.shape[0], two_d.shape[1], row0)).to(x.device)
    s = torch.tensor(float(scale(p)), dtype=torch.float32).to(x.dtype)
    out = torch.where(keep, two_d * s, torch.zeros((), dtype=x.dtype, device=x.device))
    return out if x.dim() == 2 else out[0]


# ----------------------------------------------------------------------------
# the device
# ----------------------------------------------------------------------------
def dropout_mask(p: float, seed: int, sample: int, site: int, n_rows: int, n_cols: int, device=None) -> torch.Tensor:
    """uint8[n_rows, n_cols] on the device: 1 where the element is kept (hipac_mil_dropout_mask)."""
    lib = load_mil_dropout_library()
    p = check_p(p)
    if n_rows < 1 or n_cols < 1 or n_rows * n_cols >= 1 << 31:
        raise capi.HipacError(f"mask of {n_rows} x {n_cols} refused")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise capi.HipacError("dropout_mask needs a ROCm device: there is no CPU fallback (host_mask is the host's)")
    keep = torch.empty((n_rows, n_cols), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.hipac_mil_dropout_mask(p, int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample) & _MASK32, int(site) & _MASK32, n_rows, n_cols,
                                        keep.data_ptr(), capi._stream())
    capi._check(rc, "hipac_mil_dropout_mask")
    return keep


def mil_params(sd: Dict[str, torch.Tensor], pooling: str, F: int, dev) -> capi.MilParams:
    """hipac_mil_params_t over the tensors of a MILClassifier state_dict (contiguous float32 on ``dev``)."""
    w = lambda key: capi.mil_weight_ptr(sd, key, dev)
    p = capi.MilParams()
    if pooling == "attention":
        p.attn_V_w, p.attn_V_b = w("aggregator.attn_V.weight"), w("aggregator.attn_V.bias")
        p.attn_U_w, p.attn_U_b = w("aggregator.attn_U.weight"), w("aggregator.attn_U.bias")
        p.attn_dim = int(sd["aggregator.attn_V.weight"].shape[0])
        if tuple(sd["aggregator.attn_V.weight"].shape) != (p.attn_dim, F):
            raise capi.HipacError("aggregator.attn_V.weight does not match feature_dim")
    p.fc1_w, p.fc1_b = w("classifier.0.weight"), w("classifier.0.bias")
    p.fc2_w, p.fc2_b = w("classifier.2.weight"), w("classifier.2.bias")
    p.feature_dim, p.hidden_dim = F, int(sd["classifier.0.weight"].shape[0])
    p.num_classes = int(sd["classifier.2.weight"].shape[0])
    if tuple(sd["classifier.0.weight"].shape) != (p.hidden_dim, F):
        raise capi.HipacError("classifier.0.weight does not match feature_dim")
    if tuple(sd["classifier.2.weight"].shape) != (p.num_classes, p.hidden_dim):
        raise capi.HipacError("classifier.2.weight does not match classifier.0.weight")
    return p


def mc_forward(sd: Dict[str, torch.Tensor], pooling: str, feats: torch.Tensor, offsets, p: float, seed: int, n_samples: int,
               first_sample: int = 0, want_logits: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """``n_samples`` stochastic forwards of every bag under dropout ``p`` (samples first_sample ..) and their statistics.
    ``sd``: MILClassifier state_dict tensors (float32, on the device of ``feats``); ``feats`` float32[n, F] with the rows of a
    bag contiguous; ``offsets`` int[n_bags + 1].  -> dict of device tensors: mean_prob, var_prob float64[n_bags, C]; entropy,
    expected_entropy, mutual_info float64[n_bags]; attn_mean float32[n] (attention pooling, else None); logits
    float32[n_samples, n_bags, C] (``want_logits``, else None).  Everything is checked on the host before the launch."""
    if pooling not in capi.MIL_POOLING:
        raise ValueError("Unknown pooling: choose from 'attention', 'mean', 'max'")
    lib = load_mil_dropout_library()
    if not torch.is_tensor(feats) or not feats.is_cuda:
        raise capi.HipacError("HIP path called with a CPU tensor: there is no CPU fallback (move inputs to cuda)")
    if feats.dtype != torch.float32 or feats.dim() != 2 or not feats.is_contiguous():
        raise capi.HipacError("feats must be a contiguous float32[n, feature_dim] tensor")
    p = check_p(p)
    n_samples = int(n_samples)
    if not 1 <= n_samples <= MC_MAX_SAMPLES:
        raise capi.HipacError(f"n_samples must be in 1..{MC_MAX_SAMPLES}, got {n_samples}")
    if first_sample < 0 or first_sample + n_samples > 1 << 32:
        raise capi.HipacError("first_sample .. first_sample + n_samples must stay inside 32 bits")
    n, F = int(feats.shape[0]), int(feats.shape[1])
    offs = np.asarray(offsets.detach().cpu() if torch.is_tensor(offsets) else offsets).astype(np.int64).ravel()
    if offs.size < 2 or offs[0] != 0 or bool((offs[1:] <= offs[:-1]).any()):
        raise capi.HipacError("offsets must start at 0 and increase strictly (no empty bags)")
    if int(offs[-1]) != n:
        raise capi.HipacError(f"offsets must end at the number of rows ({n}), got {int(offs[-1])}")
    n_bags, dev = offs.size - 1, feats.device
    prm = mil_params(sd, pooling, F, dev)
    pool = capi.MIL_POOLING[pooling]
    need = lib.hipac_mil_mc_workspace_bytes(C.addressof(prm), pool, n, n_bags, n_samples)
    if need == 0:
        raise capi.HipacError(f"Monte-Carlo forward of {n} rows in {n_bags} bags refused (sizes outside the kernel's limits)")
    Cn = prm.num_classes
    offs_dev = torch.from_numpy(offs.astype(np.int32)).to(dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = {"mean_prob": torch.empty((n_bags, Cn), dtype=torch.float64, device=dev),
           "var_prob": torch.empty((n_bags, Cn), dtype=torch.float64, device=dev),
           "entropy": torch.empty(n_bags, dtype=torch.float64, device=dev),
           "expected_entropy": torch.empty(n_bags, dtype=torch.float64, device=dev),
           "mutual_info": torch.empty(n_bags, dtype=torch.float64, device=dev),
           "attn_mean": torch.empty(n, dtype=torch.float32, device=dev) if pooling == "attention" else None,
           "logits": torch.empty((n_samples, n_bags, Cn), dtype=torch.float32, device=dev) if want_logits else None}
    with torch.cuda.device(dev):
        rc = lib.hipac_mil_mc_forward(C.addressof(prm), pool, feats.data_ptr(), offs_dev.data_ptr(), n, n_bags, p,
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_sample), n_samples, capi._ptr(out["logits"]),
                                      out["mean_prob"].data_ptr(), out["var_prob"].data_ptr(), out["entropy"].data_ptr(),
                                      out["expected_entropy"].data_ptr(), out["mutual_info"].data_ptr(), capi._ptr(out["attn_mean"]),
                                      ws.data_ptr(), ws.numel(), capi._stream())
    capi._check(rc, "hipac_mil_mc_forward")
    return out
