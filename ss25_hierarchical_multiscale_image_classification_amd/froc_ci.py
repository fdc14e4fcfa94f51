"""Slide-level ROC and percentile-bootstrap intervals of ``--run_evaluation`` (``--eval_roc``, ``--eval_bootstrap B``).

CAMELYON16 is scored on the lesion-level FROC and the slide-level ROC AUC, both with percentile-bootstrap intervals over
resamples of the slides (Bejnordi et al. 2017: 2 000 of them).  ``froc.py`` gives the FROC's point estimate; this module
adds the ROC of the same evaluated cases and the B replicates behind the intervals.

A replicate draws S case indices out of S with replacement (Philox, include/hipac_eval_ci.h has the draws) and is, by
definition, ``froc.computeFROC`` + ``froc.froc_score`` on the case lists with case s repeated ``counts[s]`` times, plus the
Mann-Whitney AUC of the repeated slides.  The B weighted scans run on the device (``csrc/eval_ci.hip``, one workgroup per
replicate) in integers only; everything float happens here:

  * ``build_tables`` settles the script's comparisons once -- FP probabilities as float64, TP slots as float32 against the
    thresholds rounded to float32 -- and hands the kernel ranks: the distinct values T_0 < T_1 < ... of the full table and,
    per event, the highest index at which it is counted and the index its own value contributes;
  * ``finish`` divides the integers that come back exactly as ``computeFROC`` / ``froc_score`` divide theirs, so a
    replicate equals the host composition bit for bit (tests/test_eval_ci_host.py, tests/test_gpu_eval_ci.py).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import capi
from .froc import FP_RATES

EVAL_CI_ABI_VERSION = 1  # include/hipac_eval_ci.h HIPAC_EVAL_CI_ABI_VERSION this binding was written against
MAX_CASES, MAX_EVENTS, MAX_REPLICATES, MAX_RATES, CHUNK = 4096, 1 << 24, 65536, 8, 1024
RATES4 = tuple(int(4 * r) for r in FP_RATES)  # 1/4 .. 8 FPs per slide as the kernel's integers 1 .. 32
NO_EVENT = np.iinfo(np.int32).max  # case_min_own of a case without events

# name -> (restype, argtypes); must list every symbol include/hipac_eval_ci.h declares (tests/test_eval_ci_capi_symbols.py)
EVAL_CI_SYMBOLS = {
    "hipac_eval_ci_abi_version": (C.c_int, []),
    "hipac_eval_ci_counts": (C.c_int, [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "hipac_eval_ci_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hipac_eval_ci_bootstrap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_uint64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_bound = None


def load_eval_ci_library():
    """The library of ``capi.load_library()`` with the bootstrap entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, EVAL_CI_SYMBOLS, "hipac_eval_ci_abi_version", EVAL_CI_ABI_VERSION, "eval CI ABI")
    return lib


# ---- the integer tables ---------------------------------------------------------------------------------------------


def build_tables(FROC_data, scores: Sequence[float], labels: Sequence[int]) -> Dict[str, np.ndarray]:
    """The kernel's tables (include/hipac_eval_ci.h) of ``FROC_data`` = (names, FP lists, TP arrays, numbers of tumours) and
    the slides' scores and labels (1 = tumour), as int32 arrays."""
    fps, tps, ntum = FROC_data[1], FROC_data[2], FROC_data[3]
    S = len(FROC_data[0])
    if not 1 <= S <= MAX_CASES:
        raise capi.HipacError(f"the bootstrap takes 1 .. {MAX_CASES} evaluated cases, got {S}")
    fp_val = np.asarray([float(v) for lst in fps for v in lst], np.float64)
    fp_case = np.repeat(np.arange(S), [len(lst) for lst in fps])
    tp_parts = [np.asarray(t, np.float32).ravel() for t in tps]
    tp_val = np.concatenate(tp_parts) if tp_parts else np.zeros((0,), np.float32)
    tp_case = np.repeat(np.arange(S), [p.shape[0] for p in tp_parts])
    if fp_val.shape[0] + tp_val.shape[0] > MAX_EVENTS:
        raise capi.HipacError(f"the bootstrap takes at most {MAX_EVENTS} events, got {fp_val.shape[0] + tp_val.shape[0]}")
    T = np.unique(np.concatenate([fp_val, tp_val.astype(np.float64)]))
    T32 = T.astype(np.float32)  # rounding is monotone: still sorted, with repeats where neighbours round together
    fp_own = np.searchsorted(T, fp_val)  # v >= T_i  <=>  i <= the index of v
    tp_own = np.searchsorted(T, tp_val.astype(np.float64))
    tp_hi = np.searchsorted(T32, tp_val, side="right") - 1  # slot >= (float32)T_i, compared as float32
    case = np.concatenate([2 * fp_case, 2 * tp_case + 1])
    hi, own = np.concatenate([fp_own, tp_hi]), np.concatenate([fp_own, tp_own])
    order = np.argsort(-hi, kind="stable")
    case_min_own = np.full(S, NO_EVENT, np.int64)
    np.minimum.at(case_min_own, case >> 1, own)
    sc, lab = np.asarray(scores, np.float64), np.asarray(labels, np.int64)
    if sc.shape != (S,) or lab.shape != (S,) or np.isnan(sc).any():
        raise capi.HipacError("the slide scores must be one number per evaluated case")
    by_score = np.argsort(sc, kind="stable")
    ss = sc[by_score]
    first = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))  # first position of every tie group
    group = np.cumsum(np.concatenate([[True], ss[1:] != ss[:-1]])) - 1
    bounds = np.concatenate([first, [S]])
    i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    return {"ev_case": i32(case[order]), "ev_hi": i32(hi[order]), "ev_own": i32(own[order]),
            "case_tumours": i32([int(k) for k in ntum]), "case_min_own": i32(case_min_own),
            "slide_case": i32(2 * by_score + (lab[by_score] != 0)), "slide_tie": i32(np.stack([bounds[group], bounds[group + 1]], 1)),
            "n_thresholds": int(T.shape[0])}


# ---- the device calls -----------------------------------------------------------------------------------------------


def _device(device) -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _check_replicates(B: int):
    if not 1 <= int(B) <= MAX_REPLICATES:
        raise capi.HipacError(f"the bootstrap takes 1 .. {MAX_REPLICATES} replicates per call, got {B}")


def draw_counts(seed: int, first_replicate: int, B: int, S: int, device=None) -> np.ndarray:
    """int32[B, S]: how often each case is drawn in replicates first_replicate .. first_replicate + B - 1."""
    lib = load_eval_ci_library()
    _check_replicates(B)
    dev = _device(device)
    with torch.cuda.device(dev):
        out = torch.empty((B, max(S, 0)), dtype=torch.int32, device=dev)
        capi._check(lib.hipac_eval_ci_counts(int(seed) % 2 ** 64, first_replicate, B, S, out.data_ptr(), capi._stream()),
                    "hipac_eval_ci_counts")
    return out.cpu().numpy()


def bootstrap_integers(tables: Dict[str, np.ndarray], seed: int, first_replicate: int, B: int, rates4: Sequence[int] = RATES4,
                       device=None) -> Dict[str, np.ndarray]:
    """The per-replicate integers of hipac_eval_ci_bootstrap: tp_at_rate int64[B, len(rates4)], tumours, u2 int64[B],
    n_pos, n_neg int32[B]."""
    lib = load_eval_ci_library()
    _check_replicates(B)
    dev = _device(device)
    S, n, R = tables["case_tumours"].shape[0], tables["ev_case"].shape[0], len(rates4)
    with torch.cuda.device(dev):
        d = {k: torch.from_numpy(v).to(dev) for k, v in tables.items() if isinstance(v, np.ndarray)}
        out = {"tp_at_rate": torch.empty((B, R), dtype=torch.int64, device=dev), "tumours": torch.empty(B, dtype=torch.int64, device=dev),
               "u2": torch.empty(B, dtype=torch.int64, device=dev), "n_pos": torch.empty(B, dtype=torch.int32, device=dev),
               "n_neg": torch.empty(B, dtype=torch.int32, device=dev)}
        ev = [d[k].data_ptr() if n else None for k in ("ev_case", "ev_hi", "ev_own")]
        rates = (C.c_int32 * max(R, 1))(*[int(r) for r in rates4])
        capi._check(lib.hipac_eval_ci_bootstrap(*ev, n, d["case_tumours"].data_ptr(), d["case_min_own"].data_ptr(),
                                                d["slide_case"].data_ptr(), d["slide_tie"].data_ptr(), S, int(seed) % 2 ** 64,
                                                first_replicate, B, C.cast(rates, C.c_void_p), R, out["tp_at_rate"].data_ptr(),
                                                out["tumours"].data_ptr(), out["u2"].data_ptr(), out["n_pos"].data_ptr(),
                                                out["n_neg"].data_ptr(), capi._stream()), "hipac_eval_ci_bootstrap")
        return {k: v.cpu().numpy() for k, v in out.items()}


# ---- the float work ----------------------------------------------------------------------------------------------------


def finish(ints: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """float64 per replicate: ``sensitivity_at`` [B, rates] and ``froc_score`` [B] as ``computeFROC`` + ``froc_score`` give
    them (count / float(tumours), the closing point's 0 / tumours in the maximum, so no tumour drawn gives nan), and
    ``auc`` [B] = U / (n_pos n_neg), nan where one class was not drawn."""
    tp, tum = ints["tp_at_rate"].astype(np.int64), ints["tumours"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sens = np.maximum(tp / tum[:, None], (np.zeros_like(tum) / tum)[:, None])  # np.maximum passes nan on, as max() does
        total = sens[:, 0].copy()
        for i in range(1, sens.shape[1]):  # numpy.mean's order for a handful of values: one after the other
            total = total + sens[:, i]
        pairs = ints["n_pos"].astype(np.float64) * ints["n_neg"].astype(np.float64)
        auc = (ints["u2"].astype(np.float64) * 0.5) / pairs
    return {"sensitivity_at": sens, "froc_score": total / float(sens.shape[1]), "auc": auc}


def sensitivity_at(total_FPs, total_sensitivity, rates: Sequence[float] = FP_RATES):
    """The six terms of ``froc.froc_score``: the largest sensitivity whose FP count per slide is <= the rate."""
    fps, sens = np.asarray(total_FPs, np.float64), np.asarray(total_sensitivity, np.float64)
    return [float(sens[fps <= r].max()) if (fps <= r).any() else 0.0 for r in rates]


def roc_curve(labels: Sequence[int], scores: Sequence[float]):
    """(thresholds, fpr, tpr, auc, n_pos, n_neg) over the distinct scores in descending order, after a leading (0, 0) point
    whose threshold is None; auc = the Mann-Whitney statistic with ties counted half, None (as fpr / tpr entries are nan)
    when a class is missing."""
    y, s = np.asarray(labels, np.int64) != 0, np.asarray(scores, np.float64)
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    thr = np.unique(s)[::-1]
    pos, neg = np.sort(s[y]), np.sort(s[~y])
    tp = n_pos - np.searchsorted(pos, thr, side="left")  # scores >= the threshold
    fp = n_neg - np.searchsorted(neg, thr, side="left")
    with np.errstate(divide="ignore", invalid="ignore"):
        tpr = np.concatenate([[0], tp]) / float(n_pos)
        fpr = np.concatenate([[0], fp]) / float(n_neg)
    auc = None
    if n_pos and n_neg:
        below = np.searchsorted(neg, pos, side="left")
        tied = np.searchsorted(neg, pos, side="right") - below
        auc = (float(int((2 * below + tied).sum())) * 0.5) / (float(n_pos) * float(n_neg))
    return [None] + thr.tolist(), fpr, tpr, auc, n_pos, n_neg


def read_slide_scores(path: str) -> Dict[str, float]:
    """case name -> score from lines ``name,score[,...]``; a first line whose second field is no number (the
    ``bag,probability,prediction`` header of results/mil_predictions.csv) is skipped."""
    out = {}
    with open(path) as f:
        for i, line in enumerate(f):
            elems = line.rstrip().split(",")
            if len(elems) < 2:
                if line.strip():
                    raise ValueError(f"{path}:{i + 1}: expected 'name,score', got '{line.rstrip()}'")
                continue
            try:
                out[elems[0]] = float(elems[1])
            except ValueError:
                if i:
                    raise ValueError(f"{path}:{i + 1}: '{elems[1]}' is no score") from None
    return out


def slide_scores(cases: Sequence[str], max_probs: Sequence[float], path: Optional[str] = None):
    """The score of every evaluated case: the largest detection probability (0.0 without detections), or the entry of
    ``path``; a case without a line there is an error."""
    if path is None:
        return [float(v) for v in max_probs]
    table = read_slide_scores(path)
    missing = [c for c in cases if c not in table]
    if missing:
        raise KeyError(f"{path} has no score for {', '.join(missing[:5])}{' ...' if len(missing) > 5 else ''}")
    return [table[c] for c in cases]


def _num(v):
    """A float for JSON: None for nan (an undefined quantity)."""
    return None if v is None or np.isnan(v) else float(v)


def roc_results(cases, labels, scores) -> dict:
    """The content of roc_results.json."""
    thr, fpr, tpr, auc, n_pos, n_neg = roc_curve(labels, scores)
    return {"cases": [{"case": c, "label": int(bool(y)), "score": float(s)} for c, y, s in zip(cases, labels, scores)],
            "thresholds": thr, "fpr": [_num(v) for v in fpr], "tpr": [_num(v) for v in tpr], "auc": auc, "n_pos": n_pos, "n_neg": n_neg}


def plotROC(fpr, tpr, auc, path: str) -> bool:
    """The ROC written to ``path``; False when matplotlib cannot be imported."""
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:  # noqa: BLE001 -- optional dependency
        return False
    fig, ax = plt.subplots()
    ax.plot(fpr, tpr, color="black")
    ax.plot([0, 1], [0, 1], color="grey", linestyle=":")
    ax.set_xlabel("false positive rate")
    ax.set_ylabel("true positive rate")
    ax.set_title("slide-level ROC" if auc is None else f"slide-level ROC (AUC {auc:.4f})")
    fig.savefig(path)
    plt.close(fig)
    return True


def interval(value, replicates: np.ndarray, ci: float) -> dict:
    """{value, lo, hi, undefined}: numpy.percentile of the defined (non-nan) replicates at 50 -+ ci / 2."""
    r = np.asarray(replicates, np.float64)
    ok = r[~np.isnan(r)]
    lo, hi = (np.percentile(ok, [50.0 - ci / 2.0, 50.0 + ci / 2.0]) if ok.size else (None, None))
    return {"value": _num(value), "lo": _num(lo), "hi": _num(hi), "undefined": int(r.size - ok.size)}


def bootstrap_results(fin: Dict[str, np.ndarray], point: dict, B: int, seed: int, ci: float, with_auc: bool) -> dict:
    """The content of bootstrap_results.json from the finished replicates and the point estimates ``point`` =
    {"froc_score", "sensitivity_at": [six], "auc"}."""
    res = {"replicates": int(B), "seed": int(seed), "ci": float(ci), "rates": list(FP_RATES),
           "froc_score": interval(point["froc_score"], fin["froc_score"], ci),
           "sensitivity_at": [interval(v, fin["sensitivity_at"][:, i], ci) for i, v in enumerate(point["sensitivity_at"])]}
    if with_auc:
        res["auc"] = interval(point["auc"], fin["auc"], ci)
    return res


def check_options(bootstrap: int, ci: float):
    if not 0 <= int(bootstrap) <= MAX_REPLICATES:
        raise ValueError(f"--eval_bootstrap takes 0 (off) .. {MAX_REPLICATES} replicates, got {bootstrap}")
    if not 0.0 < float(ci) < 100.0:
        raise ValueError(f"--eval_ci takes a percentage above 0 and below 100, got {ci}")


def run(cwd: str, cases, FROC_data, labels, max_probs, total_FPs, total_sensitivity, point_score: float, *, eval_roc: bool,
        slide_scores_path: Optional[str], bootstrap: int, ci: float, seed: int) -> int:
    """The part of ``froc.run_evaluation`` behind ``--eval_roc`` / ``--eval_bootstrap``: writes roc_results.json (and
    roc.png) and bootstrap_results.json into ``cwd`` and prints one line per quantity.  1 after a message when the scores
    file is unreadable or lacks a case, else 0."""
    import json

    try:
        scores = slide_scores(cases, max_probs, slide_scores_path)
    except (KeyError, ValueError, OSError) as e:
        print(f"[ERROR] --eval_slide_scores: {e.args[0] if isinstance(e, KeyError) else e}")
        return 1
    auc = None
    if eval_roc:
        res = roc_results(cases, labels, scores)
        auc = res["auc"]
        with open(os.path.join(cwd, "roc_results.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        if auc is None:
            print(f"[INFO] Slide-level ROC: {res['n_pos']} tumour and {res['n_neg']} normal cases, one class only: no AUC")
        else:
            print(f"[INFO] Slide-level ROC over {len(cases)} cases ({res['n_pos']} tumour, {res['n_neg']} normal): AUC {auc:.4f}")
        plotted = auc is not None and plotROC(res["fpr"], res["tpr"], auc, os.path.join(cwd, "roc.png"))
        print(f"[INFO] Results written to roc_results.json{' and roc.png' if plotted else ''}")
    if not bootstrap:
        return 0
    try:
        tables = build_tables(FROC_data, scores, labels)
    except capi.HipacError as e:  # more cases or events than the kernel takes
        print(f"[ERROR] --eval_bootstrap: {e}")
        return 1
    fin = finish(bootstrap_integers(tables, seed, 0, bootstrap))
    point = {"froc_score": point_score, "sensitivity_at": sensitivity_at(total_FPs, total_sensitivity), "auc": auc}
    res = bootstrap_results(fin, point, bootstrap, seed, ci, eval_roc)
    with open(os.path.join(cwd, "bootstrap_results.json"), "w") as fh:
        json.dump(res, fh, indent=1)

    def line(name, e):
        if e["lo"] is None:
            return f"[INFO] {name}: undefined in all {bootstrap} replicates"
        value = "nan" if e["value"] is None else f"{e['value']:.4f}"
        return f"[INFO] {name}: {value} ({ci:g} % CI {e['lo']:.4f} .. {e['hi']:.4f}; undefined in {e['undefined']} of {bootstrap} replicates)"

    print(line("CAMELYON16 score", res["froc_score"]))
    for r, e in zip(FP_RATES, res["sensitivity_at"]):
        print(line(f"sensitivity at {r:g} FPs per slide", e))
    if eval_roc:
        print(line("slide-level AUC", res["auc"]))
    print("[INFO] Results written to bootstrap_results.json")
    return 0
