"""Lesion detection (``--detect``): the stage between the patch classifier and ``--run_evaluation``.

The standard CAMELYON16 post-processing, which the reference never finished (src/preprocessing/pre_patches.py is a heat-map
stub around an undefined ``model``): score the slide densely with overlapping windows, build a tumour probability map, smooth
it, run non-maximum suppression, write one ``probability,x,y`` line per detection.

Geometry.  A window is 1792 / 896 / 448 / 224 pixels at levels 0..3 (``extract.PATCH_SIZES``), which is 1792 level-0 pixels
at every level.  With a cell of ``C`` level-0 pixels, level ``l`` is scanned with a stride of ``C >> l`` level-``l`` pixels
(the nominal power of two), every window covers ``K x K`` cells, ``K = 1792 / C``, and ONE cell grid ``ceil(W0 / C) x
ceil(H0 / C)`` serves all four scales -- so the levels can be fused cell by cell, the "hierarchical multiscale" step.

Everything after the logits runs on the device through include/hipac_detect.h (``csrc/detect.hip``): probabilities, one map
per level, fusion, Gaussian smoothing, NMS.  Logits never visit the host; one small copy per slide brings the detection list
back.  Every stage after the probabilities is bitwise reproducible and equal to the numpy restatement tests/detect_cpu.py.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi

DETECT_ABI_VERSION = 1  # include/hipac_detect.h HIPAC_DETECT_ABI_VERSION this binding was written against
WINDOW_L0 = 1792        # level-0 pixels under a window of any level
MAX_K, MAX_TAPS_RADIUS, MAX_NMS_RADIUS = 56, 32, 64  # HIPAC_DETECT_MAX_*
FUSE_MODES = {"mean": 0, "max": 1}  # HIPAC_DETECT_FUSE_*

# name -> (restype, argtypes); must list every symbol include/hipac_detect.h declares (tests/test_detect_capi_symbols.py)
DETECT_SYMBOLS = {
    "hipac_detect_abi_version": (C.c_int, []),
    "hipac_detect_probs": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_detect_level_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_detect_fuse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_detect_smooth": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_detect_nms_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hipac_detect_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
}

_bound = None


def load_detect_library():
    """The library of ``capi.load_library()`` with the detection entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, DETECT_SYMBOLS, "hipac_detect_abi_version", DETECT_ABI_VERSION, "detect ABI")
    return lib


# ---- geometry (host) -------------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class Geometry:
    """Cell size ``cell`` (level-0 pixels), the levels scanned, ``K`` cells per window side."""
    cell: int
    levels: Tuple[int, ...]
    K: int

    def stride(self, level: int) -> int:
        """Scan stride of ``level`` in pixels of that level: the nominal ``cell / 2^level``, not the file's measured downsample."""
        return self.cell >> level

    def grid(self, level0_size: Tuple[int, int]) -> Tuple[int, int]:
        """(gw, gh) = (ceil(W0 / cell), ceil(H0 / cell))."""
        w0, h0 = int(level0_size[0]), int(level0_size[1])
        return -(-w0 // self.cell), -(-h0 // self.cell)

    def cell_centre(self, i, j):
        """Level-0 pixel a detection at cell (i, j) is reported at: (int((i + 0.5) cell), int((j + 0.5) cell))."""
        return int((i + 0.5) * self.cell), int((j + 0.5) * self.cell)


def geometry(cell: int = 224, levels: Sequence[int] = (0, 1, 2, 3)) -> Geometry:
    """Checked geometry; ValueError (before any GPU is touched) for a cell size the window lattice cannot carry."""
    levels = tuple(sorted(set(int(l) for l in levels)))
    cell = int(cell)
    if not levels or any(l < 0 or l > 3 for l in levels):
        raise ValueError(f"detection levels must be a non-empty subset of 0..3, got {list(levels)}")
    if cell < 1 or WINDOW_L0 % cell:
        raise ValueError(f"detection cell {cell} must divide the window's {WINDOW_L0} level-0 pixels (e.g. 1792, 896, 448, 224, 112, 64, 32)")
    if WINDOW_L0 // cell > MAX_K:
        raise ValueError(f"detection cell {cell} gives {WINDOW_L0 // cell} cells per window side; at most {MAX_K} (cell >= 32)")
    for l in levels:
        if cell % (1 << l):
            raise ValueError(f"detection cell {cell} is not a multiple of 2^{l}: level {l} cannot be scanned with a whole-pixel stride")
    return Geometry(cell, levels, WINDOW_L0 // cell)


def gaussian_taps(sigma: float) -> np.ndarray:
    """float64[2 R + 1] taps of scipy's ``gaussian_filter`` (``_gaussian_kernel1d``, truncate = 4): ``exp(-k^2 / (2 sigma^2))``,
    ``R = int(4 sigma + 0.5)``, normalised.  The device gets them rounded to float32."""
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError(f"sigma {sigma} must be positive (0 skips the smoothing)")
    radius = int(4.0 * sigma + 0.5)
    if radius > MAX_TAPS_RADIUS:
        raise ValueError(f"sigma {sigma} gives a tap radius of {radius} cells; at most {MAX_TAPS_RADIUS}")
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def check_parameters(sigma: float, radius: int, max_detections: int, fuse: str):
    """ValueError for post-processing parameters the device stage refuses; called before any GPU work."""
    if fuse not in FUSE_MODES:
        raise ValueError(f"fuse must be one of {sorted(FUSE_MODES)}, got {fuse!r}")
    if sigma < 0:
        raise ValueError(f"sigma {sigma} must be >= 0")
    if sigma > 0:
        gaussian_taps(sigma)
    if not 0 <= int(radius) <= MAX_NMS_RADIUS:
        raise ValueError(f"NMS radius {radius} outside 0..{MAX_NMS_RADIUS} cells")
    if int(max_detections) < 1:
        raise ValueError(f"max_detections {max_detections} must be at least 1")


# ---- device stages ---------------------------------------------------------------------------------------------------


def tumor_probs(logits: torch.Tensor, tumor_class: int = 1) -> torch.Tensor:
    """float32[n] = 1 / (1 + exp(l_other - l_tumor)) of float32[n, 2] device logits."""
    lib = load_detect_library()
    if logits.dim() != 2 or logits.shape[1] != 2 or logits.dtype != torch.float32:
        raise capi.HipacError(f"tumor_probs needs float32[n, 2] logits, got {logits.dtype}{list(logits.shape)}")
    capi._require_gpu(logits)
    n = logits.shape[0]
    p = torch.empty(n, dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        capi._check(lib.hipac_detect_probs(logits.data_ptr() if n else None, n, tumor_class, p.data_ptr() if n else None,
                                           capi._stream()), "hipac_detect_probs")
    return p


def level_map(p: torch.Tensor, meta: torch.Tensor, level: int, geom: Geometry, grid: Tuple[int, int]):
    """(map float32[gh, gw], count int32[gh, gw]) of one level: the mean of ``p`` over the windows of ``level`` covering each
    cell.  ``meta`` int32[n, 4] = (level, x, y, label); rows of other levels are skipped on the device."""
    lib = load_detect_library()
    gw, gh = grid
    n = p.shape[0]
    if meta.shape != (n, 4) or meta.dtype != torch.int32:
        raise capi.HipacError(f"level_map needs int32[{n}, 4] meta, got {meta.dtype}{list(meta.shape)}")
    capi._require_gpu(p, meta)
    dev = p.device
    with torch.cuda.device(dev):
        origin = torch.empty((gh, gw), dtype=torch.int32, device=dev)
        out = torch.empty((gh, gw), dtype=torch.float32, device=dev)
        count = torch.empty((gh, gw), dtype=torch.int32, device=dev)
        capi._check(lib.hipac_detect_level_map(p.data_ptr() if n else None, meta.data_ptr() if n else None, n, level, geom.stride(level),
                                               geom.K, gw, gh, origin.data_ptr(), out.data_ptr(), count.data_ptr(), capi._stream()),
                    "hipac_detect_level_map")
    return out, count


def fuse_maps(maps: torch.Tensor, counts: torch.Tensor, mode: str = "mean") -> torch.Tensor:
    """float32[gh, gw] of float32[L, gh, gw] maps and int32[L, gh, gw] counts (ascending levels): per cell the mean (or the
    maximum) over the levels that have data there, 0 where none has."""
    lib = load_detect_library()
    capi._require_gpu(maps, counts)
    L, gh, gw = maps.shape
    out = torch.empty((gh, gw), dtype=torch.float32, device=maps.device)
    with torch.cuda.device(maps.device):
        capi._check(lib.hipac_detect_fuse(maps.data_ptr(), counts.data_ptr(), L, gw, gh, FUSE_MODES[mode], out.data_ptr(), capi._stream()),
                    "hipac_detect_fuse")
    return out


def smooth_map(m: torch.Tensor, sigma: float) -> torch.Tensor:
    """Separable Gaussian of a float32[gh, gw] device map, zeros outside; ``sigma`` in cells, 0 returns ``m`` itself."""
    if sigma == 0:
        return m
    lib = load_detect_library()
    capi._require_gpu(m)
    taps = np.ascontiguousarray(gaussian_taps(sigma).astype(np.float32))
    gh, gw = m.shape
    tmp, out = torch.empty_like(m), torch.empty_like(m)
    with torch.cuda.device(m.device):
        capi._check(lib.hipac_detect_smooth(m.data_ptr(), gw, gh, taps.ctypes.data, (len(taps) - 1) // 2, tmp.data_ptr(), out.data_ptr(),
                                            capi._stream()), "hipac_detect_smooth")
    return out


def nms(m: torch.Tensor, radius: int = 4, threshold: float = 0.5, max_detections: int = 2000):
    """Greedy NMS of a float32[gh, gw] device map: (p float32[k], ij int32[k, 2] = (i, j)) as numpy arrays, largest first,
    ties to the lowest raster index.  The one device-to-host copy of the detection stage (12 bytes per slot + the count)."""
    lib = load_detect_library()
    capi._require_gpu(m)
    gh, gw = m.shape
    M = int(max_detections)
    ws_bytes = lib.hipac_detect_nms_workspace_bytes(gw, gh)
    if ws_bytes == 0:
        raise capi.HipacError(f"NMS of a {gw} x {gh} map refused (gw * gh must stay below 2^31)")
    with torch.cuda.device(m.device):
        packed = torch.zeros(1 + 3 * M, dtype=torch.int32, device=m.device)  # count | p[M] | ij[M][2]: one buffer, one copy
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=m.device)
        capi._check(lib.hipac_detect_nms(m.data_ptr(), gw, gh, int(radius), float(threshold), M, packed[1:].data_ptr(),
                                         packed[1 + M:].data_ptr(), packed.data_ptr(), ws.data_ptr(), ws_bytes, capi._stream()),
                    "hipac_detect_nms")
        host = packed.cpu().numpy()
    k = int(host[0])
    return host[1:1 + k].view(np.float32).copy(), host[1 + M:1 + M + 2 * k].reshape(k, 2).copy()


# ---- the Python surface ----------------------------------------------------------------------------------------------


@dataclass
class DetectionResult:
    """Detections of one slide.  ``prob`` float32[k], ``x`` / ``y`` int64[k] level-0 pixels (numpy, largest first); ``fused``
    the fused map before smoothing and ``smoothed`` the map NMS ran on (the same tensor when sigma = 0), both float32[gh, gw]
    on the device; ``level_maps`` / ``level_counts`` per level; ``probs`` float32[n] the tumour probability of every scored
    window, in the order of ``meta`` int32[n, 4] = (level, x, y, label).  ``views``: the number of views ``probs`` is the mean
    of (test-time augmentation, ``tta.py``); ``tta_range`` float32[n] on the device, the largest minus the smallest per-view
    probability of every window, None when the windows were scored in one view."""
    geometry: Geometry
    grid: Tuple[int, int]
    prob: np.ndarray
    x: np.ndarray
    y: np.ndarray
    fused: torch.Tensor
    smoothed: torch.Tensor
    probs: torch.Tensor
    meta: torch.Tensor
    level_maps: Dict[int, torch.Tensor] = field(default_factory=dict)
    level_counts: Dict[int, torch.Tensor] = field(default_factory=dict)
    views: int = 1
    tta_range: Optional[torch.Tensor] = None


def detections_from_scores(logits, meta, level0_size: Tuple[int, int], levels: Sequence[int] = (0, 1, 2, 3), cell: int = 224,
                           fuse: str = "mean", sigma: float = 1.0, radius: int = 4, threshold: float = 0.5,
                           max_detections: int = 2000, tumor_class: int = 1, device=None) -> DetectionResult:
    """Everything after the scan: ``logits`` float32[n, 2] and ``meta`` int32[n, 4] = (level, x, y, label) as
    ``extract.score_slide`` returns them (any row order; torch or numpy, moved to the device if they are not there), of a slide
    of ``level0_size`` = (W0, H0).  ``levels`` names the levels whose rows are used.  ``logits`` float32[V, n, 2] are the
    scores of V views of every window (``score_slide(views=...)``): ``probs`` is then their mean probability
    (``tta.reduce``), ``tta_range`` is kept, and everything downstream is unchanged."""
    geom = geometry(cell, levels)
    check_parameters(sigma, radius, max_detections, fuse)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lg = torch.as_tensor(logits)
    n_views = lg.shape[0] if lg.dim() == 3 else 0  # 0: one view, the path through tumor_probs
    lg = (lg.reshape(n_views, -1, 2) if n_views else lg.reshape(-1, 2)).to(device=dev, dtype=torch.float32).contiguous()
    mt = torch.as_tensor(meta).reshape(-1, 4).to(device=dev, dtype=torch.int32).contiguous()
    if lg.shape[-2] != mt.shape[0]:
        raise capi.HipacError(f"{lg.shape[-2]} logit rows but {mt.shape[0]} meta rows")
    grid = geom.grid(level0_size)
    gw, gh = grid
    with torch.cuda.device(dev):
        tta_range = None
        if n_views:
            from . import tta

            p, tta_range = tta.reduce(lg, tumor_class, want_range=True)
        else:
            p = tumor_probs(lg, tumor_class)
        maps = torch.empty((len(geom.levels), gh, gw), dtype=torch.float32, device=dev)
        counts = torch.empty((len(geom.levels), gh, gw), dtype=torch.int32, device=dev)
        for k, level in enumerate(geom.levels):
            m, c = level_map(p, mt, level, geom, grid)
            maps[k], counts[k] = m, c
        fused = fuse_maps(maps, counts, fuse)
        smoothed = smooth_map(fused, sigma)
        prob, ij = nms(smoothed, radius, threshold, max_detections)
    x = ((ij[:, 0].astype(np.float64) + 0.5) * geom.cell).astype(np.int64)
    y = ((ij[:, 1].astype(np.float64) + 0.5) * geom.cell).astype(np.int64)
    return DetectionResult(geom, grid, prob, x, y, fused, smoothed, p, mt,
                           {l: maps[k] for k, l in enumerate(geom.levels)}, {l: counts[k] for k, l in enumerate(geom.levels)},
                           max(1, n_views), tta_range)


def range_map(result: DetectionResult, fuse: str = "mean") -> torch.Tensor:
    """float32[gh, gw] map of where the views of a test-time augmented scan disagree: ``result.tta_range`` taken through the
    ``level_map`` and ``fuse_maps`` calls the probabilities go through (per cell the mean over the covering windows of a level,
    then ``fuse`` over the levels with data).  HipacError for a result of one view."""
    if result.tta_range is None:
        raise capi.HipacError("range_map: the result has one view (detect_slide(tta=...) with rot4 or d4 keeps the range)")
    geom, (gw, gh) = result.geometry, result.grid
    dev = result.tta_range.device
    with torch.cuda.device(dev):
        maps = torch.empty((len(geom.levels), gh, gw), dtype=torch.float32, device=dev)
        counts = torch.empty((len(geom.levels), gh, gw), dtype=torch.int32, device=dev)
        for k, level in enumerate(geom.levels):
            maps[k], counts[k] = level_map(result.tta_range, result.meta, level, geom, result.grid)
        return fuse_maps(maps, counts, fuse)


@torch.no_grad()
def detect_slide(slide, net, levels: Sequence[int] = (0, 1, 2, 3), cell: int = 224, fuse: str = "mean", sigma: float = 1.0,
                 radius: int = 4, threshold: float = 0.5, max_detections: int = 2000, tumor_class: int = 1,
                 tissue=None, tta: str = "none") -> DetectionResult:
    """Dense scan of ``slide`` (``extract.DeviceSlide``) with the two-class ``net`` at every level of ``levels`` and the
    detection stage over the logits.  ``tissue`` (``tissue.TissueFilter``, default None = the whiteness test): the windows
    are chosen by the slide's Otsu tissue mask, one mask for all levels.  ``tta`` (``tta.MODES``: none, rot4, d4): score every
    window in 1, 4 or 8 views of the square and average the tumour probabilities; about as many scans as views."""
    from . import tta as tta_mod
    from .extract import score_slide

    if tta not in tta_mod.MODES:
        raise ValueError(f"tta must be one of {sorted(tta_mod.MODES)}, got {tta!r}")
    views = tta_mod.MODES[tta]
    scan_args = {"views": views} if len(views) > 1 else {}  # tta="none": the call of before, argument for argument

    geom = geometry(cell, levels)
    check_parameters(sigma, radius, max_detections, fuse)
    if net.num_classes != 2:
        raise capi.HipacError(f"detection needs a two-class network, got {net.num_classes} classes")
    if any(l >= len(slide.levels) for l in geom.levels):
        raise capi.HipacError(f"slide {slide.name} has {len(slide.levels)} levels; asked for {list(geom.levels)}")
    dev = slide.device
    logits, metas = [], []
    # one level per score_slide call: the non-lattice path of LevelWindows keeps 150 KB of pixels per kept window until its
    # level is scored, so four dense levels of a large slide held at once could reach tens of GB (an estimate from the window
    # counts, not a measurement)
    for level in geom.levels:
        _, lg, _, mt = score_slide(slide, net, levels=(level,), stride=geom.stride(level), tissue=tissue, **scan_args)
        if lg is not None and mt.shape[0]:
            logits.append(lg), metas.append(mt)
    if len(views) > 1:
        lg = torch.cat(logits, dim=1) if logits else torch.empty((len(views), 0, 2), dtype=torch.float32, device=dev)
    else:
        lg = torch.cat(logits) if logits else torch.empty((0, 2), dtype=torch.float32, device=dev)
    mt = torch.cat(metas) if metas else torch.empty((0, 4), dtype=torch.int32, device=dev)
    return detections_from_scores(lg, mt, slide.level_dimensions[0], geom.levels, cell, fuse, sigma, radius, threshold, max_detections,
                                  tumor_class, device=dev)


def save_detection_csv(path: str, result: DetectionResult) -> int:
    """One ``probability,x,y`` line per detection, the format ``froc.readCSVContent`` parses: the float32 probability with
    nine significant digits (it reads back to the same float32), integer level-0 coordinates.  Returns the number of lines."""
    with open(path, "w") as f:
        for p, x, y in zip(result.prob, result.x, result.y):
            f.write(f"{float(p):.9g},{int(x)},{int(y)}\n")
    return len(result.prob)
