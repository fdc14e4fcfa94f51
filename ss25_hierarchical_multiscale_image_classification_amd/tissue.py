"""Otsu tissue mask (``--tissue_filter otsu``): an opt-in replacement of the extractor's whiteness test.

The reference keeps a window when its mean is at most 240 (src/main.py:706-709) and has no tissue mask; that rule stays the
default and the parity path.  This module adds what CAMELYON16 pipelines usually start from: the coarsest resident level of the
slide is reduced to a thumbnail with one pixel per 32 x 32 nominal level-0 pixels, the thumbnail's saturation is thresholded with
Otsu's method, the mask is opened and dilated, and a summed-area table decides every window of every level with four reads --
before any pixel of the window is touched, so a densely scanned level resamples only the windows that hold tissue.

Everything runs on the device through include/hipac_tissue.h (``csrc/tissue.hip``); the threshold stays in device memory, so the
host does not wait for it.  Integer arithmetic except the Otsu score (IEEE double): every tensor is bit for bit the numpy
restatement tests/tissue_cpu.py.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import capi

TISSUE_ABI_VERSION = 1  # include/hipac_tissue.h HIPAC_TISSUE_ABI_VERSION this binding was written against
CELL = 32               # HIPAC_TISSUE_CELL: nominal level-0 pixels under one mask pixel
WINDOW_L0 = 1792        # HIPAC_TISSUE_WINDOW
MAX_PIXELS = 1 << 24    # HIPAC_TISSUE_MAX_PIXELS
MAX_DILATE = 8          # HIPAC_TISSUE_MAX_DILATE

# name -> (restype, argtypes); must list every symbol include/hipac_tissue.h declares (tests/test_tissue_capi_symbols.py)
TISSUE_SYMBOLS = {
    "hipac_tissue_abi_version": (C.c_int, []),
    "hipac_tissue_thumbnail": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_tissue_otsu": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_tissue_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_tissue_integral": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_tissue_window_keep": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
}

_bound = None


def load_tissue_library():
    """The library of ``capi.load_library()`` with the tissue entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, TISSUE_SYMBOLS, "hipac_tissue_abi_version", TISSUE_ABI_VERSION, "tissue ABI")
    return lib


def min_permille(min_frac: float) -> int:
    """``round(1000 * min_frac)``: the integer the device compares with."""
    return int(round(1000.0 * float(min_frac)))


def check_parameters(min_frac: float = 0.05, dilate: int = 1, sat_floor: int = 16):
    """ValueError for parameters the device stage refuses; called before any GPU work."""
    if not 0.0 <= float(min_frac) <= 1.0:  # also refuses NaN
        raise ValueError(f"tissue_min {min_frac} outside 0..1 (the fraction of a window's mask pixels that must be tissue)")
    if int(dilate) != dilate or not 0 <= int(dilate) <= MAX_DILATE:
        raise ValueError(f"tissue_dilate {dilate} outside 0..{MAX_DILATE} mask pixels")
    if int(sat_floor) != sat_floor or not 0 <= int(sat_floor) <= 255:
        raise ValueError(f"tissue_sat_floor {sat_floor} outside 0..255")


def mask_geometry(level_dimensions) -> Tuple[int, int, int, int]:
    """(Lc, f, mw, mh) of a slide with these per-level (W, H): the coarsest level, ``f = 32 >> Lc`` level pixels per mask
    pixel (the nominal power of two, not the file's measured downsample), the mask's size.  ValueError if it cannot be made."""
    lc = len(level_dimensions) - 1
    if not 0 <= lc <= 3:
        raise ValueError(f"the tissue mask needs 1..4 resident levels, got {lc + 1}")
    f = CELL >> lc
    w, h = int(level_dimensions[lc][0]), int(level_dimensions[lc][1])
    mw, mh = -(-w // f), -(-h // f)
    if mw < 1 or mh < 1 or mw * mh >= MAX_PIXELS:
        raise ValueError(f"tissue mask {mw} x {mh} refused (need at least one pixel and mw * mh < 2^24)")
    return lc, f, mw, mh


@dataclass(frozen=True)
class TissueFilter:
    """The parameters of the filter, as every scan entry point takes them (``tissue=TissueFilter(...)``; None = the
    reference's whiteness test).  ``min_frac``: the smallest tissue fraction of a window's mask rectangle; ``dilate``: radius
    of the final dilation in mask pixels; ``sat_floor``: the threshold never goes below it (a blank slide has only noise to
    split); ``opening``: the 3 x 3 opening (the command line always opens)."""
    min_frac: float = 0.05
    dilate: int = 1
    sat_floor: int = 16
    opening: bool = True

    def __post_init__(self):
        check_parameters(self.min_frac, self.dilate, self.sat_floor)

    @property
    def min_permille(self) -> int:
        return min_permille(self.min_frac)

    def mask(self, slide) -> "TissueMask":
        """The slide's mask for these parameters; made once per slide and parameter set."""
        return TissueMask.from_slide(slide, self.sat_floor, self.dilate, self.opening)

    def window_keep(self, slide, xy: torch.Tensor, level: int):
        return self.mask(slide).window_keep(xy, level, self.min_frac)


# ---- device stages ---------------------------------------------------------------------------------------------------


def thumbnail(level: torch.Tensor, width: int, f: int):
    """(thumb uint8[mh, mw, 3], sat uint8[mh, mw], hist int32[256]) of a uint8[H, Wpad, 3] device level whose first ``width``
    pixels of a row are the image (``DeviceSlide.levels``: Wpad a multiple of 16)."""
    lib = load_tissue_library()
    capi._require_gpu(level)
    if level.dtype != torch.uint8 or level.dim() != 3 or level.shape[2] != 3:
        raise capi.HipacError("level must be uint8[H, Wpad, 3]")
    H, wp, _ = level.shape
    f = int(f)
    if f not in (4, 8, 16, 32):
        raise capi.HipacError(f"thumbnail factor {f} must be 4, 8, 16 or 32")
    mw, mh = -(-int(width) // f), -(-H // f)
    dev = level.device
    thumb = torch.empty((mh, mw, 3), dtype=torch.uint8, device=dev)
    sat = torch.empty((mh, mw), dtype=torch.uint8, device=dev)
    hist = torch.empty((256,), dtype=torch.int32, device=dev)  # uint32 bit pattern; counts stay below 2^24
    with torch.cuda.device(dev):
        capi._check(lib.hipac_tissue_thumbnail(level.data_ptr(), int(width), H, wp * 3, f, thumb.data_ptr(), sat.data_ptr(),
                                               hist.data_ptr(), capi._stream()), "hipac_tissue_thumbnail")
    return thumb, sat, hist


def otsu(hist: torch.Tensor, sat_floor: int = 16) -> torch.Tensor:
    """int32[2] = (Otsu's threshold, max(it, sat_floor)) of an int32[256] device histogram, left on the device."""
    lib = load_tissue_library()
    capi._require_gpu(hist)
    if hist.dtype != torch.int32 or tuple(hist.shape) != (256,):
        raise capi.HipacError(f"otsu needs an int32[256] histogram, got {hist.dtype}{list(hist.shape)}")
    thr = torch.empty((2,), dtype=torch.int32, device=hist.device)
    with torch.cuda.device(hist.device):
        capi._check(lib.hipac_tissue_otsu(hist.data_ptr(), int(sat_floor), thr.data_ptr(), capi._stream()), "hipac_tissue_otsu")
    return thr


def clean_mask(sat: torch.Tensor, thresholds: torch.Tensor, dilate: int = 1, opening: bool = True) -> torch.Tensor:
    """uint8[mh, mw] of 0 / 1: ``sat > thresholds[1]`` (read on the device), opened 3 x 3 if ``opening``, dilated by ``dilate``."""
    lib = load_tissue_library()
    capi._require_gpu(sat, thresholds)
    if sat.dtype != torch.uint8 or sat.dim() != 2 or thresholds.dtype != torch.int32 or tuple(thresholds.shape) != (2,):
        raise capi.HipacError("clean_mask needs a uint8[mh, mw] saturation map and int32[2] thresholds")
    mh, mw = sat.shape
    tmp, mask = torch.empty_like(sat), torch.empty_like(sat)
    with torch.cuda.device(sat.device):
        capi._check(lib.hipac_tissue_mask(sat.data_ptr(), mw, mh, thresholds.data_ptr(), int(bool(opening)), int(dilate), tmp.data_ptr(),
                                          mask.data_ptr(), capi._stream()), "hipac_tissue_mask")
    return mask


def integral(mask: torch.Tensor) -> torch.Tensor:
    """int32[mh + 1, mw + 1] summed-area table of a uint8[mh, mw] device mask."""
    lib = load_tissue_library()
    capi._require_gpu(mask)
    if mask.dtype != torch.uint8 or mask.dim() != 2:
        raise capi.HipacError("integral needs a uint8[mh, mw] mask")
    mh, mw = mask.shape
    table = torch.empty((mh + 1, mw + 1), dtype=torch.int32, device=mask.device)
    with torch.cuda.device(mask.device):
        capi._check(lib.hipac_tissue_integral(mask.data_ptr(), mw, mh, table.data_ptr(), capi._stream()), "hipac_tissue_integral")
    return table


def window_keep(table: torch.Tensor, xy: torch.Tensor, level: int, permille: int):
    """(keep uint8[n], count int32[n]) of the windows with origins ``xy`` int32[n, 2] (pixels of ``level``)."""
    lib = load_tissue_library()
    capi._require_gpu(table, xy)
    if table.dtype != torch.int32 or table.dim() != 2 or xy.dtype != torch.int32 or xy.dim() != 2 or xy.shape[1] != 2:
        raise capi.HipacError("window_keep needs an int32[mh + 1, mw + 1] table and int32[n, 2] origins")
    n = xy.shape[0]
    keep = torch.empty((n,), dtype=torch.uint8, device=table.device)
    count = torch.empty((n,), dtype=torch.int32, device=table.device)
    with torch.cuda.device(table.device):
        capi._check(lib.hipac_tissue_window_keep(table.data_ptr(), table.shape[1] - 1, table.shape[0] - 1, xy.data_ptr() if n else None, n,
                                                 int(level), int(permille), keep.data_ptr() if n else None,
                                                 count.data_ptr() if n else None, capi._stream()), "hipac_tissue_window_keep")
    return keep, count


# ---- the Python surface ----------------------------------------------------------------------------------------------


class TissueMask:
    """The mask of one slide, on the device: ``thumb`` uint8[mh, mw, 3], ``sat`` uint8[mh, mw], ``hist`` int32[256],
    ``thresholds`` int32[2] = (Otsu, effective), ``mask`` uint8[mh, mw], ``table`` int32[mh + 1, mw + 1].  ``kept`` collects,
    per level, (device count of kept windows, number of windows) of the scans that used it -- for the report line."""

    def __init__(self, level: int, f: int, thumb, sat, hist, thresholds, mask, table):
        self.level, self.f = level, f
        self.thumb, self.sat, self.hist, self.thresholds, self.mask, self.table = thumb, sat, hist, thresholds, mask, table
        self.kept: Dict[int, Tuple[torch.Tensor, int]] = {}

    @classmethod
    def from_slide(cls, slide, sat_floor: int = 16, dilate: int = 1, opening: bool = True) -> "TissueMask":
        check_parameters(0.0, dilate, sat_floor)
        key = (int(sat_floor), int(dilate), bool(opening))
        cache = slide.__dict__.setdefault("_tissue_masks", {})
        if key not in cache:
            try:
                lc, f, _, _ = mask_geometry(slide.level_dimensions)
            except ValueError as e:
                raise capi.HipacError(f"slide {slide.name}: {e}") from None
            thumb, sat, hist = thumbnail(slide.levels[lc], slide.level_dimensions[lc][0], f)
            thr = otsu(hist, sat_floor)
            mask = clean_mask(sat, thr, dilate, opening)
            cache[key] = cls(lc, f, thumb, sat, hist, thr, mask, integral(mask))
        return cache[key]

    def window_keep(self, xy: torch.Tensor, level: int, min_frac: float = 0.05):
        """(keep uint8[n], count int32[n]) for windows of ``level`` at ``xy`` int32[n, 2]."""
        check_parameters(min_frac, 0, 0)
        return window_keep(self.table, xy, level, min_permille(min_frac))

    def report(self) -> str:
        """One line: both thresholds, the tissue fraction, kept / total windows per level scanned (reads the device)."""
        t, te = self.thresholds.cpu().tolist()
        frac = float(self.mask.sum(dtype=torch.int64).item()) / self.mask.numel()
        per_level = ", ".join(f"L{l} {int(k.item())}/{n}" for l, (k, n) in sorted(self.kept.items()))
        return (f"otsu threshold {t} (effective {te}), tissue {100.0 * frac:.1f}% of {self.mask.shape[1]} x {self.mask.shape[0]} mask pixels"
                + (f", windows kept {per_level}" if per_level else ""))
