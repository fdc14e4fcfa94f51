"""Test-time augmentation of the detector (``--detect_tta``): every window is scored in several of the eight views of the
square -- the four rotations by 90 degrees, each with and without a mirror -- and its tumour probability is the mean over
the views.  H&E tissue has no preferred orientation and the patch classifier is trained with random flips and rotations
(``augment.py``); averaging the views is standard practice in CAMELYON16 detectors (Liu et al. 2017).

Device code: include/hipac_tta.h (``csrc/tta.hip``).  ``view`` permutes the bytes of uint8[n, 224, 224, 3] patches; ``reduce``
turns float32[V, n, 2] logits into the mean probability per window and the range over the views.  ``score_views`` is the
loop ``extract.score_slide`` runs: the trunk is deterministic and position-independent, so a view costs one pass over the
bytes of a slice and then the forward that exists.  tests/tta_cpu.py is the numpy restatement.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import capi

TTA_ABI_VERSION = 1  # include/hipac_tta.h HIPAC_TTA_ABI_VERSION this binding was written against
SIDE, VIEWS = 224, 8  # HIPAC_TTA_SIDE, HIPAC_TTA_VIEWS
# view = r + 4 f: mirror the columns if f, then r quarter turns counter-clockwise
MODES = {"none": (0,), "rot4": (0, 1, 2, 3), "d4": tuple(range(8))}
INVERSE = (0, 3, 2, 1, 4, 5, 6, 7)  # view INVERSE[v] undoes view v

# name -> (restype, argtypes); must list every symbol include/hipac_tta.h declares (tests/test_tta_capi_symbols.py)
TTA_SYMBOLS = {
    "hipac_tta_abi_version": (C.c_int, []),
    "hipac_tta_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_tta_reduce": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_bound = None


def load_tta_library():
    """The library of ``capi.load_library()`` with the entry points of hipac_tta.h bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, TTA_SYMBOLS, "hipac_tta_abi_version", TTA_ABI_VERSION, "tta ABI")
    return lib


def check_views(views: Sequence[int]):
    """The views as a tuple; ValueError unless they are distinct, in 0..7 and begin with the untouched view 0."""
    vs = tuple(int(v) for v in views)
    if not vs or vs[0] != 0 or len(set(vs)) != len(vs) or any(v < 0 or v >= VIEWS for v in vs):
        raise ValueError(f"views must be distinct numbers in 0..{VIEWS - 1} that begin with 0, got {list(views)}")
    return vs


def view(x: torch.Tensor, v: int, out: torch.Tensor = None) -> torch.Tensor:
    """View ``v`` of uint8[n, 224, 224, 3] device patches, into ``out`` (same shape, no overlap with ``x``) or a new tensor.
    Equal to ``np.rot90(x[:, :, ::-1] if v >= 4 else x, v % 4, axes=(1, 2))``."""
    lib = load_tta_library()
    if x.dtype != torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (SIDE, SIDE, 3):
        raise capi.HipacError(f"view needs uint8[n, {SIDE}, {SIDE}, 3] patches, got {x.dtype}{list(x.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.uint8 or out.shape != x.shape or out.device != x.device:
        raise capi.HipacError(f"view: out must be uint8{list(x.shape)} on {x.device}, got {out.dtype}{list(out.shape)} on {out.device}")
    capi._require_gpu(x, out)
    n = x.shape[0]
    if not 0 <= int(v) < VIEWS:
        raise capi.HipacError(f"view {v} outside 0..{VIEWS - 1}")
    if n == 0:  # an empty tensor has no address to pass
        return out
    with torch.cuda.device(x.device):
        capi._check(lib.hipac_tta_view(x.data_ptr(), n, int(v), out.data_ptr(), capi._stream()), "hipac_tta_view")
    return out


def reduce(logits: torch.Tensor, tumor_class: int = 1, want_range: bool = False):
    """float32[n] mean tumour probability of float32[V, n, 2] device logits: the per-view probabilities of
    ``detect.tumor_probs`` added in ascending view order and divided once.  ``want_range``: (mean, max - min over the views)."""
    lib = load_tta_library()
    if logits.dim() != 3 or logits.shape[2] != 2 or logits.dtype != torch.float32 or not 1 <= logits.shape[0] <= VIEWS:
        raise capi.HipacError(f"reduce needs float32[V, n, 2] logits with 1 <= V <= {VIEWS}, got {logits.dtype}{list(logits.shape)}")
    capi._require_gpu(logits)
    V, n = logits.shape[0], logits.shape[1]
    p = torch.empty(n, dtype=torch.float32, device=logits.device)
    rng = torch.empty(n, dtype=torch.float32, device=logits.device) if want_range else None
    with torch.cuda.device(logits.device):
        capi._check(lib.hipac_tta_reduce(logits.data_ptr() if n else None, V, n, int(tumor_class), p.data_ptr() if n else None,
                                         rng.data_ptr() if want_range and n else None, capi._stream()), "hipac_tta_reduce")
    return (p, rng) if want_range else p


@torch.no_grad()
def score_views(net: capi.PackedResNet18, patches_u8: torch.Tensor, views: Sequence[int], fwd_batch: int = 8192, want_labels: bool = False):
    """(feats float32[n, 512], logits float32[V, n, 2]) of uint8[n, 224, 224, 3] device patches under ``views`` (which begin
    with 0); with ``want_labels`` a third element, the int64[n] labels of view 0.

    ``feats`` and ``logits[0]`` come from the forward over the untouched buffer: view 0 is a copy, so it is never
    materialised.  For every slice of ``fwd_batch`` patches and every other view, the slice is transformed into the view
    buffer of ``net`` (grow-only, sized to ONE slice: 1.23 GB at 8 192) and forwarded without features.  Everything is
    queued on the caller's stream, so the next view may overwrite the buffer the previous forward read without any
    extra ordering."""
    vs = check_views(views)
    if net.num_classes != 2:
        raise capi.HipacError(f"score_views needs a two-class network, got {net.num_classes} classes")
    n = patches_u8.shape[0]
    dev = patches_u8.device
    step = max(1, int(fwd_batch))
    feats = torch.empty((n, 512), dtype=torch.float32, device=dev)
    logits = torch.empty((len(vs), n, 2), dtype=torch.float32, device=dev)
    labels = torch.empty((n,), dtype=torch.int64, device=dev) if want_labels else None
    for lo in range(0, n, step):
        end = min(n, lo + step)
        f, l, lab = net.forward(patches_u8[lo:end], want_feats=True, want_logits=True, want_labels=want_labels)
        feats[lo:end], logits[0, lo:end] = f, l
        if want_labels:
            labels[lo:end] = lab
        for k, v in enumerate(vs[1:], start=1):
            vb = view(patches_u8[lo:end], v, out=net.view_buffer(end - lo, dev))
            logits[k, lo:end] = net.forward(vb, want_feats=False, want_logits=True)[1]
    return (feats, logits, labels) if want_labels else (feats, logits)
