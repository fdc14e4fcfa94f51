"""HED stain augmentation (``--aug_hed SIGMA``): an opt-in stage of the device input pipelines of the training loops.

CAMELYON16 comes from two centres and two scanners.  ``--stain_norm macenko`` treats that on the inference side; this is the
training side: every training view gets a random affine map of its own in optical-density space, which scales (alpha) and shifts
(beta) the concentrations of haematoxylin, eosin and DAB on the Ruifrok-Johnston basis (Tellez et al. 2018 / 2019).  The
reference has no such stage; it is off by default.  The draws and the 3 x 3 map are made here on the host in float64, the per-pixel
arithmetic runs inside the colour kernel of ``hipac_augment_views_hed`` (csrc/augment.hip, csrc/augment_hed.h) with the integer
optical-density table of the Macenko stage.  include/hipac_augment_hed.h is the definition; tests/augment_hed_cpu.py restates it
and the device equals it bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import capi

AUGMENT_HED_ABI_VERSION = 1  # include/hipac_augment_hed.h HIPAC_AUGMENT_HED_ABI_VERSION this binding was written against
PAYLOAD = 12                 # HIPAC_AUGMENT_HED_PAYLOAD: A[3][3] row-major, then bq[3]
MAX_SIGMA = 0.5
OD_MAX = 22713               # HIPAC_STAIN_OD_MAX
OUT = 224
STREAM_KEY = 11              # the HED draws come from np.random.default_rng([seed, rank, STREAM_KEY]), a stream of their own

# rows H, E, D: the optical densities of the three stains per unit of concentration (Ruifrok and Johnston 2001)
RGB_FROM_HED = ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11), (0.27, 0.57, 0.78))
# its inverse, printed once with repr: od . HED_FROM_RGB = the concentrations of H, E, D
HED_FROM_RGB = ((1.8779827368521353, -1.0076786862855645, -0.5561158181996246),
                (-0.06590806222356332, 1.1347303724996625, -0.1355217986283712),
                (-0.6019073634392891, -0.4804141884970579, 1.5735880719641926))

# name -> (restype, argtypes); must list every symbol include/hipac_augment_hed.h declares (tests/test_augment_hed_capi_symbols.py)
AUGMENT_HED_SYMBOLS = {
    "hipac_augment_hed_abi_version": (C.c_int, []),
    "hipac_augment_views_hed": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "hipac_augment_hed_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_bound = None


def load_augment_hed_library():
    """The library of ``capi.load_library()`` with the HED entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, AUGMENT_HED_SYMBOLS, "hipac_augment_hed_abi_version", AUGMENT_HED_ABI_VERSION, "augment HED ABI")
    return lib


def check_sigma(sigma) -> float:
    """``sigma`` as a float in 0 .. 0.5; ValueError otherwise (also for NaN)."""
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"aug_hed sigma {sigma!r} is not a number") from None
    if not 0.0 <= s <= MAX_SIGMA:
        raise ValueError(f"aug_hed sigma {sigma} outside 0 .. {MAX_SIGMA} (0 = off, 0.05 light, 0.2 strong)")
    return s


def hed_rng(seed: int, rank: int = 0) -> np.random.Generator:
    """The generator of a loader's HED draws: separate from the loaders' own streams, which therefore never move."""
    return np.random.default_rng([int(seed), int(rank), STREAM_KEY])


def maps_from_draws(alpha, beta) -> np.ndarray:
    """float64 [n, 12] payloads of alpha, beta float64 [n, 3] (H, E, D): one rounding per operation, in the header's order."""
    a = np.asarray(alpha, np.float64).reshape(-1, 3)
    b = np.asarray(beta, np.float64).reshape(-1, 3)
    R, Ri = RGB_FROM_HED, HED_FROM_RGB
    out = np.empty((a.shape[0], PAYLOAD), np.float64)
    T = [[Ri[i][j] * a[:, j] for j in range(3)] for i in range(3)]
    for c in range(3):
        for k in range(3):
            out[:, 3 * c + k] = (T[k][0] * R[0][c] + T[k][1] * R[1][c]) + T[k][2] * R[2][c]
        out[:, 9 + c] = 4096.0 * ((b[:, 0] * R[0][c] + b[:, 1] * R[1][c]) + b[:, 2] * R[2][c])
    return out


def draw_maps(n: int, sigma: float, rng: np.random.Generator) -> np.ndarray:
    """float64 [n, 12]: per view six draws from ``rng``, alpha_k ~ U(1 - sigma, 1 + sigma) for H, E, D, then beta_k ~
    U(-sigma, sigma); then the view's map."""
    s = check_sigma(sigma)
    lo = np.array([1.0 - s] * 3 + [-s] * 3, np.float64)
    hi = np.array([1.0 + s] * 3 + [s] * 3, np.float64)
    d = rng.uniform(lo, hi, (int(n), 6))
    return maps_from_draws(d[:, :3], d[:, 3:])


def identity_maps(n: int) -> np.ndarray:
    """float64 [n, 12]: A = I, bq = 0 -- the payload that leaves every byte as it is."""
    out = np.zeros((int(n), PAYLOAD), np.float64)
    out[:, 0] = out[:, 4] = out[:, 8] = 1.0
    return out


def _tables():
    od = np.rint(4096.0 * np.log(256.0 / (np.arange(256) + 1.0))).astype(np.int64)
    q = np.arange(OD_MAX + 1, dtype=np.int64)
    lo = np.searchsorted(-od, -q, side="left")  # the smallest v with od[v] <= q (od decreases)
    up = np.maximum(lo - 1, 0)
    inv = np.where((lo > 0) & (od[up] - q < q - od[lo]), up, lo).astype(np.uint8)  # the nearer one, ties to the larger v
    return od, inv


def host_apply(images_u8, maps) -> np.ndarray:
    """The stage in numpy: uint8 [n, ..., 3] images under float64 [n, 12] maps.  For tests and inspection, not a hot path."""
    img = np.asarray(images_u8)
    m = np.asarray(maps, np.float64)
    if img.dtype != np.uint8 or img.ndim < 2 or img.shape[-1] != 3 or m.shape != (img.shape[0], PAYLOAD):
        raise ValueError("host_apply needs uint8 [n, ..., 3] images and float64 [n, 12] maps")
    od, inv = _tables()
    out = np.empty_like(img)
    for i in range(img.shape[0]):
        o = od[img[i]].astype(np.float64)
        for c in range(3):
            t = np.rint(((m[i, 3 * c] * o[..., 0] + m[i, 3 * c + 1] * o[..., 1]) + m[i, 3 * c + 2] * o[..., 2]) + m[i, 9 + c])
            t = np.where(t >= 0.0, np.minimum(t, float(OD_MAX)), 0.0)  # a NaN counts as 0, as on the device
            out[i, ..., c] = inv[t.astype(np.int64)]
    return out


def check_maps(maps, n: int) -> np.ndarray:
    """``maps`` as contiguous float64 [n, 12], every entry finite; HipacError otherwise."""
    m = np.ascontiguousarray(maps, dtype=np.float64)
    if m.shape != (n, PAYLOAD):
        raise capi.HipacError(f"HED maps must be float64 [{n}, {PAYLOAD}], got {m.shape}")
    if not np.isfinite(m).all():
        raise capi.HipacError("HED maps must be finite")
    return m


class PinnedRing:
    """float64 host buffers an asynchronous copy reads from: four pinned slots, an event per slot says when its copy has run (an
    asynchronous copy from pageable memory would make the host wait for everything queued before it)."""

    def __init__(self, slots: int = 4):
        self._next, self._buf, self._ev = -1, [None] * slots, [None] * slots

    def stage(self, array: np.ndarray) -> tuple:
        """(slot, pinned tensor holding ``array``); waits only if the copy that last read this slot has not run yet."""
        slot = self._next = (self._next + 1) % len(self._buf)
        if self._ev[slot] is not None:
            self._ev[slot].synchronize()
        flat = array.reshape(-1)
        if self._buf[slot] is None or self._buf[slot].numel() < flat.size:
            self._buf[slot] = torch.empty((flat.size,), dtype=torch.float64).pin_memory()
        host = self._buf[slot][:flat.size]
        host.numpy()[:] = flat
        return slot, host

    def mark(self, slot: int, device):
        """Record, after the enqueue, the point on the current stream behind which the slot is free again."""
        self._ev[slot] = torch.cuda.Event()
        self._ev[slot].record(torch.cuda.current_stream(device))


_ring = None


def apply(images_dev: torch.Tensor, maps) -> torch.Tensor:
    """The stage alone, in place on a device tensor uint8 [n, 224, 224, 3] (``hipac_augment_hed_apply``); returns it."""
    global _ring
    lib = load_augment_hed_library()
    capi._require_gpu(images_dev)
    if images_dev.dtype != torch.uint8 or images_dev.dim() != 4 or tuple(images_dev.shape[1:]) != (OUT, OUT, 3):
        raise capi.HipacError("apply needs uint8 [n, 224, 224, 3] images")
    n = int(images_dev.shape[0])
    m = check_maps(maps, n)
    if _ring is None:
        _ring = PinnedRing()
    slot, host = _ring.stage(m)
    scratch = torch.empty((n, PAYLOAD), dtype=torch.float64, device=images_dev.device)
    with torch.cuda.device(images_dev.device):
        capi._check(lib.hipac_augment_hed_apply(images_dev.data_ptr(), n, host.data_ptr(), scratch.data_ptr(), capi._stream()),
                    "hipac_augment_hed_apply")
        _ring.mark(slot, images_dev.device)
    return images_dev


def describe(sigma: float) -> str:
    """The one line ``main.py`` prints."""
    return (f"--aug_hed: HED stain augmentation of every training view on the device, sigma {sigma:g} "
            f"(alpha ~ U({1.0 - sigma:g}, {1.0 + sigma:g}), beta ~ U({-sigma:g}, {sigma:g}) per stain; validation is not augmented)")

