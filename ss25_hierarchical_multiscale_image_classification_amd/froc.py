"""CAMELYON16 FROC evaluation (``--run_evaluation``; reference: src/utils/evaluation_FROC.py, src/main.py:1168-1225).

The reference's functions by name and meaning.  The image work runs on the device through include/hipac_eval.h
(``csrc/froc.hip``): the evaluation mask (thresholded exact EDT, hole fill, 8-connected labelling, bit for bit the
scipy / scikit-image pipeline), the integer region moments behind the ITC list, and the label under every detection.
What stays on the host is bookkeeping over a few thousand detections, kept in the reference's order because its
quirks decide the numbers:

  * ``TP_probs`` is float32[max_label] and keeps a slot for every ITC label (it stays 0);
  * a detection updates a label only if ``p > TP_probs[label - 1]``, a comparison against the float32 value;
  * a hit on an ITC label is neither a TP nor an FP; in a non-tumour case every detection is an FP;
  * the FROC thresholds are ``sorted(set(FPs + TPs))[1:]`` and the TP counts compare float32 values.

Additions: ``froc_score`` (the challenge's six-point score, the mean sensitivity at 1/4 .. 8 FPs per slide), the mask
sources of ``load_case_mask`` (grayscale tiled TIFF masks or the XML annotations rasterised with the extractor's rule)
and ``run_evaluation``, the CLI body, which also writes ``froc_results.json`` (and ``froc.png``).  The slide-level ROC and the
bootstrap intervals of ``--eval_roc`` / ``--eval_bootstrap`` are in ``froc_ci.py``.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi

EVAL_ABI_VERSION = 1  # include/hipac_eval.h HIPAC_EVAL_ABI_VERSION this binding was written against
L0_RESOLUTION = 0.243  # src/main.py:1191-1192
EVALUATION_MASK_LEVEL = 5
FP_RATES = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0)  # FPs per slide of the CAMELYON16 score

# name -> (restype, argtypes); must list every symbol include/hipac_eval.h declares (tests/test_eval_capi_symbols.py)
EVAL_SYMBOLS = {
    "hipac_eval_abi_version": (C.c_int, []),
    "hipac_eval_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hipac_eval_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "hipac_eval_region_moments": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_eval_lookup": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}

_bound = None


def load_eval_library():
    """The library of ``capi.load_library()`` with the evaluation entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, EVAL_SYMBOLS, "hipac_eval_abi_version", EVAL_ABI_VERSION, "eval ABI")
    return lib


def eval_threshold(resolution: float, level: int) -> float:
    """Distance threshold in level pixels: 75 um (five tumour cells) around every annotation (:31)."""
    return 75 / (resolution * pow(2, level) * 2)


def itc_threshold(resolution: float, level: int) -> float:
    """Largest major axis of an ITC in level pixels, 275 um (:57); 35.36 at level 5."""
    return 275 / (resolution * pow(2, level))


class EvaluationMask:
    """Device labels int32[H, W] (0 = background, 1..n) and their count ``n``."""

    def __init__(self, labels: torch.Tensor, n: int):
        self.labels = labels
        self.n = n

    @property
    def shape(self) -> Tuple[int, int]:
        return tuple(self.labels.shape)

    def numpy(self) -> np.ndarray:
        return self.labels.cpu().numpy()


def evaluation_mask(mask_u8, resolution: float = L0_RESOLUTION, level: int = EVALUATION_MASK_LEVEL,
                    device: Optional[torch.device] = None) -> EvaluationMask:
    """computeEvaluationMask of one mask level (uint8[H, W], numpy or torch; channel 0 of the mask image): the labels
    of ``binary_fill_holes(edt(255 - mask) < eval_threshold)``, 8-connected, in raster order, on the device."""
    lib = load_eval_library()
    m = torch.as_tensor(mask_u8)
    if m.dtype != torch.uint8 or m.dim() != 2:
        raise capi.HipacError(f"evaluation_mask needs a uint8[H, W] mask, got {m.dtype}{list(m.shape)}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if m.device != dev:
        m = m.to(dev)
    if m.stride(1) != 1:
        m = m.contiguous()
    H, W = m.shape
    ws_bytes = lib.hipac_eval_workspace_bytes(W, H)
    if ws_bytes == 0:
        raise capi.HipacError(f"evaluation mask of {W} x {H} pixels refused (W * H must stay below 2^31)")
    with torch.cuda.device(dev):
        labels = torch.empty((H, W), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        capi._check(lib.hipac_eval_mask(m.data_ptr(), W, H, m.stride(0), eval_threshold(resolution, level), labels.data_ptr(),
                                        count.data_ptr(), ws.data_ptr(), ws_bytes, capi._stream()), "hipac_eval_mask")
        n = int(count.item())
    return EvaluationMask(labels, n)


def computeEvaluationMask(mask, resolution: float = L0_RESOLUTION, level: int = EVALUATION_MASK_LEVEL) -> EvaluationMask:
    """The reference's entry point: ``mask`` is a ``*_Mask.tif`` path (read at ``level``, channel 0) or the level itself."""
    if isinstance(mask, (str, os.PathLike)):
        from .tiff_pyramid import read_mask_level

        mask = read_mask_level(os.fspath(mask), level)
    return evaluation_mask(mask, resolution, level)


def region_moments(em: EvaluationMask) -> np.ndarray:
    """int64[n, 6] = (count, sum r, sum c, sum r^2, sum c^2, sum r c) of labels 1..n."""
    lib = load_eval_library()
    out = torch.zeros((em.n, 6), dtype=torch.int64, device=em.labels.device)
    if em.n:
        H, W = em.shape
        with torch.cuda.device(em.labels.device):
            capi._check(lib.hipac_eval_region_moments(em.labels.data_ptr(), W, H, em.n, out.data_ptr(), capi._stream()),
                        "hipac_eval_region_moments")
    return out.cpu().numpy()


def major_axis_lengths(moments: np.ndarray) -> List[float]:
    """scikit-image's ``major_axis_length`` = 4 sqrt(largest eigenvalue of the normalised inertia tensor), from the integer
    moments: the central moments are taken exactly as Python ints (n^2 times the covariance), one rounding after that."""
    out = []
    for n, sr, sc, srr, scc, src in (tuple(int(v) for v in row) for row in moments):
        arr, acc, arc = n * srr - sr * sr, n * scc - sc * sc, n * src - sr * sc
        lam = (float(arr + acc) + math.sqrt((arr - acc) ** 2 + 4 * arc * arc)) / (2.0 * n * n)
        out.append(4.0 * math.sqrt(max(lam, 0.0)))
    return out


def computeITCList(evaluation_mask: EvaluationMask, resolution: float = L0_RESOLUTION,
                   level: int = EVALUATION_MASK_LEVEL) -> List[int]:
    """Labels whose major axis is below ``itc_threshold`` (isolated tumour cells, :38-62)."""
    thr = itc_threshold(resolution, level)
    return [i + 1 for i, ax in enumerate(major_axis_lengths(region_moments(evaluation_mask))) if ax < thr]


def readCSVContent(csvDIR: str):
    """(Probs, Xcorr, Ycorr) of a detection CSV, one ``p,x,y`` per line (:67-88)."""
    probs, xs, ys = [], [], []
    with open(csvDIR) as f:
        for line in f:
            elems = line.rstrip().split(",")
            probs.append(float(elems[0]))
            xs.append(int(elems[1]))
            ys.append(int(elems[2]))
    return probs, xs, ys


def lookup_labels(em: EvaluationMask, Xcorr: Sequence[int], Ycorr: Sequence[int], level: int) -> np.ndarray:
    """int32[n]: the label under every level-0 point, ``labels[int(y / 2**level), int(x / 2**level)]``, 0 outside."""
    lib = load_eval_library()
    n = len(Xcorr)
    if n == 0:
        return np.zeros((0,), np.int32)
    dev = em.labels.device
    xy = torch.from_numpy(np.stack([np.asarray(Xcorr, np.int64), np.asarray(Ycorr, np.int64)], 1)).to(dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    H, W = em.shape
    with torch.cuda.device(dev):
        capi._check(lib.hipac_eval_lookup(em.labels.data_ptr(), W, H, level, xy.data_ptr(), n, out.data_ptr(), capi._stream()),
                    "hipac_eval_lookup")
    return out.cpu().numpy()


def compute_FP_TP_Probs(Ycorr, Xcorr, Probs, is_tumor, evaluation_mask: Optional[EvaluationMask], Isolated_Tumor_Cells,
                        level: int):
    """(FP_probs, TP_probs, num_of_tumors, detection_summary, FP_summary) of one case (:91-154).  ``evaluation_mask`` may
    be None (or 0, as the reference passes) for a non-tumour case."""
    max_label = evaluation_mask.n if isinstance(evaluation_mask, EvaluationMask) else 0
    hits = lookup_labels(evaluation_mask, Xcorr, Ycorr, level) if is_tumor and max_label else np.zeros(len(Xcorr), np.int32)
    return fp_tp_from_hits(hits, Xcorr, Ycorr, Probs, is_tumor, max_label, Isolated_Tumor_Cells)


def fp_tp_from_hits(hits, Xcorr, Ycorr, Probs, is_tumor, max_label: int, Isolated_Tumor_Cells):
    """The bookkeeping of ``compute_FP_TP_Probs`` once the label under every detection (``hits``) is known, in detection
    order."""
    itc = set(int(i) for i in Isolated_Tumor_Cells)
    FP_probs = []
    TP_probs = np.zeros((max_label,), dtype=np.float32)
    detection_summary = {f"Label {i}": [] for i in range(1, max_label + 1) if i not in itc}
    FP_summary = {}
    for p, x, y, hit in zip(Probs, Xcorr, Ycorr, np.asarray(hits).tolist()):
        if not is_tumor or hit == 0:
            FP_summary[f"FP {len(FP_probs)}"] = [p, x, y]
            FP_probs.append(p)
        elif hit not in itc and p > TP_probs[hit - 1]:  # against the float32 slot: p is rounded to float32 first
            detection_summary[f"Label {hit}"] = [p, x, y]
            TP_probs[hit - 1] = p
    return FP_probs, TP_probs, max_label - len(Isolated_Tumor_Cells), detection_summary, FP_summary


def computeFROC(FROC_data):
    """(total_FPs, total_sensitivity) over all cases (:157-185).  ``FROC_data`` = (case names, FP lists, TP arrays, numbers
    of tumours).  The reference's O(N^2) threshold loop as sort + searchsorted, same thresholds and comparisons: FP
    probabilities compare as float64, the float32 TP array against each threshold rounded to float32."""
    names, fps, tps, ntum = FROC_data[0], FROC_data[1], FROC_data[2], FROC_data[3]
    fp = np.sort(np.asarray([float(v) for lst in fps for v in lst], np.float64))
    tp_parts = [np.asarray(t, np.float32).ravel() for t in tps]
    tp = np.sort(np.concatenate(tp_parts)) if tp_parts else np.zeros((0,), np.float32)
    thresholds = np.unique(np.concatenate([fp, tp.astype(np.float64)]))[1:]
    fp_counts = fp.shape[0] - np.searchsorted(fp, thresholds, side="left")
    tp_counts = tp.shape[0] - np.searchsorted(tp, thresholds.astype(np.float32), side="left")
    total_fp = np.append(fp_counts.astype(np.int64), 0)
    total_tp = np.append(tp_counts.astype(np.int64), 0)
    with np.errstate(divide="ignore", invalid="ignore"):  # no tumour at all: the reference's array division gives nan too
        return total_fp / float(len(names)), total_tp / float(sum(int(k) for k in ntum))


def froc_score(total_FPs, total_sensitivity, rates: Sequence[float] = FP_RATES) -> float:
    """Addition (not in the reference's script): the CAMELYON16 score, the mean over ``rates`` of the largest sensitivity
    whose average FP count per slide is <= the rate (0 where there is none)."""
    fps, sens = np.asarray(total_FPs, np.float64), np.asarray(total_sensitivity, np.float64)
    vals = [float(sens[fps <= r].max()) if (fps <= r).any() else 0.0 for r in rates]
    return float(np.mean(vals))


def plotFROC(total_FPs, total_sensitivity, path: str) -> bool:
    """The reference's plot, written to ``path`` instead of shown; False when matplotlib cannot be imported."""
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:  # noqa: BLE001 -- optional dependency
        return False
    fig, ax = plt.subplots()
    ax.plot(total_FPs, total_sensitivity, color="black")
    ax.set_xlabel("mean false positives per slide")
    ax.set_ylabel("lesion detection sensitivity")
    ax.set_title("FROC")
    fig.savefig(path)
    plt.close(fig)
    return True


# ---- mask sources and the CLI body ---------------------------------------------------------------------------------


def mask_source(data_root: str, case: str):
    """("tif", path) of ``test/mask/<case>_Mask.tif``, else ("xml", path) of ``test/mask/annotations/<case>.xml``, else None."""
    tif = os.path.join(data_root, "test", "mask", case + "_Mask.tif")
    if os.path.exists(tif):
        return "tif", tif
    xml = os.path.join(data_root, "test", "mask", "annotations", case + ".xml")
    if os.path.exists(xml):
        return "xml", xml
    return None


def load_case_mask(data_root: str, case: str, source, level: int) -> np.ndarray:
    """uint8[H, W] mask level of a case: the TIFF mask's level ``level`` (channel 0), or the XML polygons rasterised with
    the extractor's rule at (ceil(W0 / 2^level), ceil(H0 / 2^level)), W0 x H0 from ``test/img/<case>.tif``'s header."""
    from .tiff_pyramid import TiffPyramid, read_mask_level

    kind, path = source
    if kind == "tif":
        return read_mask_level(path, level)
    from .extract import parse_annotation_xml, rasterize_mask

    img = os.path.join(data_root, "test", "img", case + ".tif")
    if not os.path.exists(img):
        raise FileNotFoundError(f"slide '{img}' (its level-0 size places the annotation) not found")
    W0, H0 = TiffPyramid(img).dimensions
    d = 2 ** level
    return rasterize_mask(parse_annotation_xml(path), (-(-W0 // d), -(-H0 // d)), (W0, H0))


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_jsonable(x) for x in v]
    if isinstance(v, (np.floating, float)):
        return float(v)
    if isinstance(v, (np.integer, int)):
        return int(v)
    return v


def froc_results(names, FROC_data, detection_summaries, FP_summaries, total_FPs, total_sensitivity) -> dict:
    """The content of froc_results.json."""
    return _jsonable({
        "cases": [{"case": n, "FP_probs": f, "TP_probs": t, "num_of_tumors": k, "detection_summary": d, "FP_summary": s}
                  for n, f, t, k, d, s in zip(names, FROC_data[1], FROC_data[2], FROC_data[3], detection_summaries, FP_summaries)],
        "total_FPs": total_FPs,
        "total_sensitivity": total_sensitivity,
        "froc_score": froc_score(total_FPs, total_sensitivity),
        "froc_score_rates": list(FP_RATES),
    })


def run_evaluation(data_root: str, cwd: Optional[str] = None, resolution: float = L0_RESOLUTION,
                   level: int = EVALUATION_MASK_LEVEL, *, eval_roc: bool = False, slide_scores: Optional[str] = None,
                   bootstrap: int = 0, ci: float = 95.0, seed: int = 0) -> int:
    """``--run_evaluation``: score ``cwd/models/first_model/model_predictions_csv/*.csv`` against the masks under
    ``data_root/test/mask``; print the curve and the score, write froc_results.json (and froc.png) into ``cwd``.
    ``eval_roc`` adds the slide-level ROC of the same cases (roc_results.json, roc.png; the score of a case is its largest
    detection probability, or its entry in the file ``slide_scores``), ``bootstrap`` > 0 the percentile intervals at ``ci``
    percent over that many resamples of the cases keyed by ``seed`` (bootstrap_results.json): ``froc_ci.py``.  Without
    them nothing else is written or printed."""
    from . import froc_ci

    froc_ci.check_options(bootstrap, ci)
    cwd = os.getcwd() if cwd is None else cwd
    print("[INFO] Running CAMELYON16 evaluation script.")
    mask_folder = os.path.join(data_root, "test", "mask")
    results_folder = os.path.join(cwd, "models", "first_model", "model_predictions_csv")
    if not os.path.exists(mask_folder):
        print(f"[ERROR] Evaluation mask folder '{mask_folder}' not found. Please generate TIFF masks from XML annotations first.")
        return 1
    if not os.path.exists(results_folder):
        print(f"[ERROR] Model results folder '{results_folder}' not found. Please run your detection model first.")
        return 1
    names, fps, tps, ntum, dets, fpsum = [], [], [], [], [], []
    labels, max_probs = [], []  # the slide-level ROC's inputs, over the same cases
    for file in sorted(f for f in os.listdir(results_folder) if f.endswith(".csv")):
        case = file[:-4]
        print(f"Evaluating Performance on image: {case}", flush=True)
        Probs, Xcorr, Ycorr = readCSVContent(os.path.join(results_folder, file))
        source = mask_source(data_root, case)
        is_tumor = case[0:5].lower() == "tumor" or source is not None
        em, itc = None, []
        if is_tumor:
            if source is None:
                print(f"[WARNING] Mask TIFF '{os.path.join(mask_folder, case + '_Mask.tif')}' not found for tumor case. Skipping.")
                continue
            try:
                mask = load_case_mask(data_root, case, source, level)
            except Exception as e:  # noqa: BLE001 -- too few levels, a missing slide header: this case only
                print(f"[ERROR] Could not read the mask of {case} ({source[1]}): {type(e).__name__}: {e}. Skipping.")
                continue
            em = evaluation_mask(mask, resolution, level)
            itc = computeITCList(em, resolution, level)
        f, t, k, d, s = compute_FP_TP_Probs(Ycorr, Xcorr, Probs, is_tumor, em, itc, level)
        names.append(file), fps.append(f), tps.append(t), ntum.append(k), dets.append(d), fpsum.append(s)
        labels.append(int(is_tumor)), max_probs.append(max(Probs) if Probs else 0.0)
    if not names:
        print("[WARNING] No cases processed for FROC evaluation.")
        return 0
    FROC_data = (names, fps, tps, ntum)
    total_FPs, total_sensitivity = computeFROC(FROC_data)
    res = froc_results(names, FROC_data, dets, fpsum, total_FPs, total_sensitivity)
    with open(os.path.join(cwd, "froc_results.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    plotted = plotFROC(total_FPs, total_sensitivity, os.path.join(cwd, "froc.png"))
    print(f"[INFO] FROC over {len(names)} cases ({sum(ntum)} tumours, {sum(len(f) for f in fps)} false positives): "
          f"{len(total_FPs)} points, sensitivity {float(total_sensitivity[0]):.4f} at {float(total_FPs[0]):.3f} FPs per slide")
    print(f"[INFO] CAMELYON16 score (mean sensitivity at 1/4, 1/2, 1, 2, 4, 8 FPs per slide): {res['froc_score']:.4f}")
    print(f"[INFO] Results written to froc_results.json{' and froc.png' if plotted else ''}")
    if eval_roc or bootstrap:
        return froc_ci.run(cwd, [n[:-4] for n in names], FROC_data, labels, max_probs, total_FPs, total_sensitivity, res["froc_score"],
                           eval_roc=eval_roc, slide_scores_path=slide_scores, bootstrap=bootstrap, ci=ci, seed=seed)
    return 0
