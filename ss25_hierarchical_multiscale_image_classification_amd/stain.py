"""Macenko stain normalisation (``--stain_norm macenko``): an opt-in stage that maps a slide's H&E colours to a target appearance
before anything else reads its pixels.

The reference has no such stage; it is off by default and off in parity runs.  The stain vectors are fitted on the coarsest
resident level (Macenko et al. 2009: the plane of the two largest principal directions of the tissue pixels' optical densities, the
extreme angles in it, the 99th-percentile concentrations) and every resident level is then mapped in place, pixel by pixel, with
one 3 x 3 matrix in optical-density space.  Everything runs on the device through include/hipac_stain.h (``csrc/stain.hip``); the
fit stays in device memory, so the host does not wait for it.  Integer optical densities (a table), integer sums and histograms,
IEEE double for the small matrices: every tensor is bit for bit the numpy restatement tests/stain_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import json
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import capi

STAIN_ABI_VERSION = 1   # include/hipac_stain.h HIPAC_STAIN_ABI_VERSION this binding was written against
Q = 12                  # HIPAC_STAIN_Q
OD_MAX = 22713          # HIPAC_STAIN_OD_MAX
ANGLE_BINS = 4096       # HIPAC_STAIN_ANGLE_BINS
CONC_BINS = 4096        # HIPAC_STAIN_CONC_BINS
MAX_ALPHA = 499         # HIPAC_STAIN_MAX_ALPHA
HE_REF = ((0.5626, 0.2159), (0.7201, 0.8012), (0.4062, 0.5581))  # the usual Macenko target: columns H, E
MAXC_REF = (1.9705, 1.0308)

_IMG = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]  # img .. beta_q
# name -> (restype, argtypes); must list every symbol include/hipac_stain.h declares (tests/test_stain_capi_symbols.py)
STAIN_SYMBOLS = {
    "hipac_stain_abi_version": (C.c_int, []),
    "hipac_stain_od_table": (C.c_int, [C.c_void_p]),
    "hipac_stain_moments": (C.c_int, [*_IMG, C.c_void_p, C.c_void_p]),
    "hipac_stain_basis": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_stain_angle_hist": (C.c_int, [*_IMG, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_stain_vectors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_stain_conc_hist": (C.c_int, [*_IMG, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_stain_matrix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hipac_stain_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_bound = None


def load_stain_library():
    """The library of ``capi.load_library()`` with the stain entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, STAIN_SYMBOLS, "hipac_stain_abi_version", STAIN_ABI_VERSION, "stain ABI")
    return lib


def od_table():
    """The library's optical-density table as a list of 256 ints (host only)."""
    buf = (C.c_int32 * 256)()
    capi._check(load_stain_library().hipac_stain_od_table(buf), "hipac_stain_od_table")
    return list(buf)


def alpha_permille(alpha: float) -> int:
    """``round(10 * alpha)``: the percentile of the angle histogram in whole permille, the integer the device ranks with."""
    return int(round(10.0 * float(alpha)))


def beta_q(beta: float) -> int:
    """``round(beta * 2^12)``: the optical-density threshold of a tissue pixel in the table's units."""
    return int(round(float(beta) * (1 << Q)))


def check_target(target) -> Tuple[Tuple[Tuple[float, float], ...], Tuple[float, float]]:
    """(HE 3 x 2, maxC 2) as tuples of floats from ``None`` (the default target) or a (HE, maxC) pair; ValueError otherwise."""
    if target is None:
        return HE_REF, MAXC_REF
    try:
        he, maxc = target
        he = tuple(tuple(float(x) for x in row) for row in he)
        maxc = tuple(float(x) for x in maxc)
    except (TypeError, ValueError):
        raise ValueError("stain target must be (HE 3 x 2, maxC 2)") from None
    if len(he) != 3 or any(len(r) != 2 for r in he) or len(maxc) != 2:
        raise ValueError("stain target must be (HE 3 x 2, maxC 2)")
    if not all(math.isfinite(x) for r in he for x in r) or not all(math.isfinite(x) and x > 0 for x in maxc):
        raise ValueError("stain target: HE must be finite and maxC finite and > 0")
    return he, maxc


def check_parameters(alpha: float = 1.0, beta: float = 0.15, target=None):
    """ValueError for parameters the device stage refuses; called before any GPU work."""
    if not 0.0 < float(alpha) < 50.0 or not 1 <= alpha_permille(alpha) <= MAX_ALPHA:  # also refuses NaN
        raise ValueError(f"stain_alpha {alpha} outside 0.1..49.9 percent (the percentile of the stain angles, in steps of 0.1)")
    if not 0.0 < float(beta) <= 1.0:
        raise ValueError(f"stain_beta {beta} outside (0, 1] (the smallest optical density of a tissue pixel)")
    check_target(target)


def load_target(path: str):
    """The (HE, maxC) target of a file ``--stain_save_fit`` wrote; ValueError if it does not hold one."""
    try:
        with open(path) as f:
            d = json.load(f)
        target = (d["HE"], d["maxC"])
    except (OSError, ValueError, KeyError, TypeError) as e:
        raise ValueError(f"stain target {path}: {type(e).__name__}: {e}") from None
    if not d.get("status", 1):
        raise ValueError(f"stain target {path}: its fit failed (status 0)")
    return check_target(target)


# ---- device stages ---------------------------------------------------------------------------------------------------


def _image_args(level: torch.Tensor, width: int, mask: Optional[torch.Tensor], f: Optional[int], bq: int):
    capi._require_gpu(level, mask)
    if level.dtype != torch.uint8 or level.dim() != 3 or level.shape[2] != 3:
        raise capi.HipacError("level must be uint8[H, Wpad, 3]")
    H, wp, _ = level.shape
    if mask is not None and (mask.dtype != torch.uint8 or mask.dim() != 2):
        raise capi.HipacError("the tissue mask must be uint8[mh, mw]")
    mh, mw = (mask.shape if mask is not None else (0, 0))
    return [level.data_ptr(), int(width), H, wp * 3, capi._ptr(mask), int(mw), int(mh), int(f or 0), int(bq)]


def moments(level: torch.Tensor, width: int, bq: int, mask: Optional[torch.Tensor] = None, f: Optional[int] = None) -> torch.Tensor:
    """int64[10] = n, S_c, S_cc' of the tissue pixels of a uint8[H, Wpad, 3] device level (``DeviceSlide.levels``)."""
    lib = load_stain_library()
    args = _image_args(level, width, mask, f, bq)
    out = torch.empty((10,), dtype=torch.int64, device=level.device)
    with torch.cuda.device(level.device):
        capi._check(lib.hipac_stain_moments(*args, out.data_ptr(), capi._stream()), "hipac_stain_moments")
    return out


def basis(mom: torch.Tensor):
    """(basis float64[2, 3], status int32[1]) of int64[10] device moments."""
    lib = load_stain_library()
    capi._require_gpu(mom)
    if mom.dtype != torch.int64 or tuple(mom.shape) != (10,):
        raise capi.HipacError("basis needs int64[10] moments")
    bas = torch.empty((2, 3), dtype=torch.float64, device=mom.device)
    st = torch.empty((1,), dtype=torch.int32, device=mom.device)
    with torch.cuda.device(mom.device):
        capi._check(lib.hipac_stain_basis(mom.data_ptr(), bas.data_ptr(), st.data_ptr(), capi._stream()), "hipac_stain_basis")
    return bas, st


def angle_hist(level: torch.Tensor, width: int, bq: int, bas: torch.Tensor, mask=None, f=None) -> torch.Tensor:
    """int32[4096] (uint32 bit pattern): the tissue pixels' angles in the plane ``bas`` float64[2, 3]."""
    lib = load_stain_library()
    args = _image_args(level, width, mask, f, bq)
    capi._require_gpu(bas)
    if bas.dtype != torch.float64 or tuple(bas.shape) != (2, 3):
        raise capi.HipacError("angle_hist needs a float64[2, 3] basis")
    hist = torch.empty((ANGLE_BINS,), dtype=torch.int32, device=level.device)
    with torch.cuda.device(level.device):
        capi._check(lib.hipac_stain_angle_hist(*args, bas.data_ptr(), hist.data_ptr(), capi._stream()), "hipac_stain_angle_hist")
    return hist


def vectors(hist: torch.Tensor, bas: torch.Tensor, basis_status: torch.Tensor, permille: int):
    """(he_p float64[12] = HE[3][2], P[2][3]; status int32[1])."""
    lib = load_stain_library()
    capi._require_gpu(hist, bas, basis_status)
    if (hist.dtype != torch.int32 or tuple(hist.shape) != (ANGLE_BINS,) or bas.dtype != torch.float64 or bas.numel() != 6
            or basis_status.dtype != torch.int32 or basis_status.numel() != 1):
        raise capi.HipacError("vectors needs an int32[4096] histogram, a float64[2, 3] basis and its int32[1] status")
    he_p = torch.empty((12,), dtype=torch.float64, device=hist.device)
    st = torch.empty((1,), dtype=torch.int32, device=hist.device)
    with torch.cuda.device(hist.device):
        capi._check(lib.hipac_stain_vectors(hist.data_ptr(), bas.data_ptr(), basis_status.data_ptr(), int(permille), he_p.data_ptr(),
                                            st.data_ptr(), capi._stream()), "hipac_stain_vectors")
    return he_p, st


def conc_hist(level: torch.Tensor, width: int, bq: int, he_p: torch.Tensor, mask=None, f=None) -> torch.Tensor:
    """int32[2, 4096] (uint32 bit pattern): the tissue pixels' stain concentrations over [0, 8) OD."""
    lib = load_stain_library()
    args = _image_args(level, width, mask, f, bq)
    capi._require_gpu(he_p)
    if he_p.dtype != torch.float64 or tuple(he_p.shape) != (12,):
        raise capi.HipacError("conc_hist needs float64[12] = HE, P")
    hist = torch.empty((2, CONC_BINS), dtype=torch.int32, device=level.device)
    with torch.cuda.device(level.device):
        capi._check(lib.hipac_stain_conc_hist(*args, he_p.data_ptr(), hist.data_ptr(), capi._stream()), "hipac_stain_conc_hist")
    return hist


def matrix(chist: torch.Tensor, he_p: torch.Tensor, vec_status: torch.Tensor, target=None):
    """(m_maxc float64[11] = M[3][3], maxC[2]; status int32[1]) for the target (HE, maxC), None = the default."""
    lib = load_stain_library()
    capi._require_gpu(chist, he_p, vec_status)
    if (chist.dtype != torch.int32 or tuple(chist.shape) != (2, CONC_BINS) or he_p.dtype != torch.float64 or he_p.numel() != 12
            or vec_status.dtype != torch.int32 or vec_status.numel() != 1):
        raise capi.HipacError("matrix needs int32[2, 4096] histograms, float64[12] = HE, P and their int32[1] status")
    he, maxc = check_target(target)
    tg = (C.c_double * 8)(*[x for row in he for x in row], *maxc)
    m = torch.empty((11,), dtype=torch.float64, device=chist.device)
    st = torch.empty((1,), dtype=torch.int32, device=chist.device)
    with torch.cuda.device(chist.device):
        capi._check(lib.hipac_stain_matrix(chist.data_ptr(), he_p.data_ptr(), vec_status.data_ptr(), tg, m.data_ptr(), st.data_ptr(),
                                           capi._stream()), "hipac_stain_matrix")
    return m, st


def apply(level: torch.Tensor, width: int, m: torch.Tensor, status: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Map the first ``width`` pixels of every row of ``level`` uint8[H, Wpad, 3] with ``m`` float64[>= 9] into ``out`` (same shape;
    None = in place; its other bytes are left as they are).  ``status`` int32[1] = 0 copies the pixels."""
    lib = load_stain_library()
    out = level if out is None else out
    capi._require_gpu(level, out, m, status)
    if level.dtype != torch.uint8 or level.dim() != 3 or level.shape[2] != 3 or out.dtype != torch.uint8 or out.shape != level.shape:
        raise capi.HipacError("apply needs uint8[H, Wpad, 3] images of one shape")
    if m.dtype != torch.float64 or m.numel() < 9 or status.dtype != torch.int32 or status.numel() != 1:
        raise capi.HipacError("apply needs a float64[>= 9] matrix and an int32[1] status")
    H, wp, _ = level.shape
    with torch.cuda.device(level.device):
        capi._check(lib.hipac_stain_apply(level.data_ptr(), out.data_ptr(), int(width), H, wp * 3, m.data_ptr(), status.data_ptr(),
                                          capi._stream()), "hipac_stain_apply")
    return out


# ---- the Python surface ----------------------------------------------------------------------------------------------


class StainFit:
    """The fit of one slide, on the device: ``moments`` int64[10], ``basis`` float64[2, 3], ``angle_hist`` int32[4096], ``he_p``
    float64[12] = HE[3][2], P[2][3], ``conc_hist`` int32[2, 4096], ``m_maxc`` float64[11] = M[3][3], maxC[2]; the three stages'
    ``basis_status``, ``vec_status``, ``status`` int32[1]."""

    def __init__(self, level: int, **tensors):
        self.level = level
        self.__dict__.update(tensors)

    def to_dict(self) -> dict:
        """{"HE": 3 x 2, "maxC": 2, "n", "status"} as Python numbers (reads the device)."""
        he_p, m_maxc = self.he_p.cpu().tolist(), self.m_maxc.cpu().tolist()
        return {"HE": [he_p[0:2], he_p[2:4], he_p[4:6]], "maxC": m_maxc[9:11], "n": int(self.moments[0].item()),
                "status": int(self.status.item())}

    def report(self) -> str:
        """One line: HE, maxC, the number of tissue pixels and the status (reads the device)."""
        d = self.to_dict()
        he = "; ".join(f"{r[0]:.4f} {r[1]:.4f}" for r in d["HE"])
        how = "ok" if d["status"] else "0: no two stains found, pixels unchanged"
        return f"macenko HE [{he}], maxC [{d['maxC'][0]:.4f} {d['maxC'][1]:.4f}], n {d['n']} tissue pixels of level {self.level}, status {how}"


@dataclass(frozen=True)
class StainNorm:
    """The parameters of the normalisation: ``alpha`` the percentile of the stain angles in percent, ``beta`` the smallest optical
    density of a tissue pixel, ``target`` (HE 3 x 2, maxC 2) or None for the usual Macenko reference."""
    alpha: float = 1.0
    beta: float = 0.15
    target: Optional[tuple] = None

    def __post_init__(self):
        check_parameters(self.alpha, self.beta, self.target)
        if self.target is not None:
            object.__setattr__(self, "target", check_target(self.target))  # hashable, comparable

    def _tissue_key(self, tissue):
        return None if tissue is None else (int(tissue.sat_floor), int(tissue.dilate), bool(tissue.opening))

    def fit(self, slide, tissue=None) -> StainFit:
        """The slide's fit for these parameters on its coarsest resident level, restricted to the tissue mask of ``tissue``
        (``tissue.TissueFilter``) when given; made once per slide, parameter set and mask."""
        key = (self, self._tissue_key(tissue))
        cache = slide.__dict__.setdefault("_stain_fits", {})
        if key not in cache:
            if slide.__dict__.get("_stain_norm") is not None:
                raise capi.HipacError(f"slide {slide.name}: already normalised; a fit would no longer see its own stains")
            lc = len(slide.levels) - 1
            level, width = slide.levels[lc], slide.level_dimensions[lc][0]
            mask = f = None
            if tissue is not None:
                tm = tissue.mask(slide)
                mask, f = tm.mask, tm.f
            bq, pm = beta_q(self.beta), alpha_permille(self.alpha)
            mom = moments(level, width, bq, mask, f)
            bas, bs = basis(mom)
            ah = angle_hist(level, width, bq, bas, mask, f)
            he_p, vs = vectors(ah, bas, bs, pm)
            ch = conc_hist(level, width, bq, he_p, mask, f)
            m_maxc, st = matrix(ch, he_p, vs, self.target)
            cache[key] = StainFit(lc, moments=mom, basis=bas, basis_status=bs, angle_hist=ah, he_p=he_p, vec_status=vs, conc_hist=ch,
                                  m_maxc=m_maxc, status=st)
        return cache[key]

    def normalize(self, slide, tissue=None) -> StainFit:
        """Fit, then map every resident level of ``slide`` in place, once.  With ``tissue`` the slide's tissue mask is made first,
        from the original pixels, and restricts the fit.  Call it right after the slide is opened, before anything derived from
        its pixels is kept (level planes, scans).  A second call with the same parameters does nothing; different ones raise."""
        key = (self, self._tissue_key(tissue))
        done = slide.__dict__.get("_stain_norm")
        if done is not None:
            if done[0] != key:
                raise capi.HipacError(f"slide {slide.name}: already normalised with other parameters")
            return done[1]
        fit = self.fit(slide, tissue)
        for level, (width, _) in zip(slide.levels, slide.level_dimensions):
            apply(level, width, fit.m_maxc, fit.status)
        slide.__dict__["_stain_norm"] = (key, fit)
        return fit
