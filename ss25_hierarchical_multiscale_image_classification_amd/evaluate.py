"""Patch-level evaluation of a saved classifier (``--eval_patches``): the reference's ``--evaluate`` stage (src/main.py:974-1015),
which prints the accuracy on the validation patches, with the quantities of its src/utils/metrics.py, the thresholded softmax
of its src/utils/uncertainty.py, a patch-level ROC / AUC and average precision, a per-slide table and percentile intervals from
a bootstrap over the validation SLIDES (patches of one slide are not independent; resampling patches would give intervals that
are far too narrow).

The network scores every batch on the HIP inference path; ``detect.tumor_probs`` turns the logits into tumour probabilities;
everything after that is integers (include/hipac_evaluate.h, ``csrc/evaluate.hip``): per slide and true class a histogram of
the probability over 4096 equal bins, per slide the confusion counts, and per bootstrap replicate the weighted confusion counts
and twice the Mann-Whitney U of the weighted histograms.  The floats are made here, on the host, from those integers, so
the result is bitwise reproducible and equal to the numpy restatement tests/eval_patches_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import capi, froc_ci

EVALUATE_ABI_VERSION = 1  # include/hipac_evaluate.h HIPAC_EVALUATE_ABI_VERSION this binding was written against
BINS, MAX_GROUPS, MAX_REPLICATES = 4096, 4096, 65536  # HIPAC_EVALUATE_*
DEFAULT_WEIGHTS = os.path.join("src", "models", "resnet18_patch_classifier.pth")  # where --train saves (src/main.py:533)
QUANTITIES = ("accuracy", "precision", "recall", "f1_score", "auc")  # what the bootstrap reports

# name -> (restype, argtypes); must list every symbol include/hipac_evaluate.h declares (tests/test_evaluate_capi_symbols.py)
EVALUATE_SYMBOLS = {
    "hipac_evaluate_abi_version": (C.c_int, []),
    "hipac_evaluate_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "hipac_evaluate_bootstrap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
}

_bound = None


def load_evaluate_library():
    """The library of ``capi.load_library()`` with the evaluation entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, EVALUATE_SYMBOLS, "hipac_evaluate_abi_version", EVALUATE_ABI_VERSION, "evaluate ABI")
    return lib


class EvaluateError(Exception):
    """A refusal of ``evaluate_patches`` with the exit status the command line answers it with."""

    def __init__(self, message: str, status: int):
        super().__init__(message)
        self.status = status


# ---- the device tables -------------------------------------------------------------------------------------------------


class PatchTally:
    """The running tables of hipac_evaluate_accumulate for ``G`` slides: ``hist`` [G, 2, 4096], ``conf`` [G, 4] = (TN, FP, FN,
    TP) and ``n_bad`` [1].  The words are uint32; torch holds them as int32 (the same bits; every count stays below 2^31)."""

    def __init__(self, G: int, device=None):
        if not 1 <= int(G) <= MAX_GROUPS:
            raise capi.HipacError(f"the patch tally takes 1 .. {MAX_GROUPS} slides, got {G}")
        load_evaluate_library()
        self.G = int(G)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.hist = torch.zeros((self.G, 2, BINS), dtype=torch.int32, device=self.device)
        self.conf = torch.zeros((self.G, 4), dtype=torch.int32, device=self.device)
        self.n_bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add(self, p: torch.Tensor, pred: torch.Tensor, label: torch.Tensor, group: torch.Tensor):
        """One batch: ``p`` float32[n] on the device, ``pred`` / ``label`` (0 or 1) and ``group`` (slide index) of n rows each."""
        lib = load_evaluate_library()
        if p.dim() != 1 or p.dtype != torch.float32:
            raise capi.HipacError(f"PatchTally.add needs float32[n] probabilities, got {p.dtype}{list(p.shape)}")
        n = int(p.shape[0])
        pred = pred.to(self.device, torch.uint8).contiguous()
        label = label.to(self.device, torch.uint8).contiguous()
        group = group.to(self.device, torch.int32).contiguous()
        if not (pred.shape == label.shape == group.shape == (n,)):
            raise capi.HipacError("PatchTally.add: p, pred, label and group must hold one entry per row")
        capi._require_gpu(p)
        ptr = lambda t: t.data_ptr() if n else None  # noqa: E731
        with torch.cuda.device(self.device):
            capi._check(lib.hipac_evaluate_accumulate(ptr(p), ptr(pred), ptr(label), ptr(group), n, self.G, self.hist.data_ptr(),
                                                      self.conf.data_ptr(), self.n_bad.data_ptr(), capi._stream()),
                        "hipac_evaluate_accumulate")

    def all_reduce(self):
        """Sum the three tables over the ranks, one all-reduce each (integer sums: the order does not matter)."""
        from . import dist as hdist

        if not hdist.active():
            return
        import torch.distributed as tdist

        for t in (self.hist, self.conf, self.n_bad):
            if tdist.get_backend() == "gloo":  # gloo reduces on the host
                h = t.cpu()
                tdist.all_reduce(h)
                t.copy_(h)
            else:
                tdist.all_reduce(t)

    def tables(self) -> Dict[str, np.ndarray]:
        """The tables on the host: hist int64[G, 2, 4096], conf int64[G, 4], n_bad int."""
        u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
        return {"hist": u32(self.hist), "conf": u32(self.conf), "n_bad": int(u32(self.n_bad)[0])}


def check_contract(hist: np.ndarray):
    """The caller's contract of hipac_evaluate_bootstrap: G * (the most rows of one slide) < 2^31."""
    G = hist.shape[0]
    most = int(hist.reshape(G, -1).sum(1).max())
    if G * most >= 2 ** 31:
        raise capi.HipacError(f"the slide bootstrap needs G * (the most patches of one slide) < 2^31; got {G} slides and {most} patches")


def bootstrap_integers(tally: PatchTally, seed: int, first_replicate: int, B: int) -> Dict[str, np.ndarray]:
    """The per-replicate integers of hipac_evaluate_bootstrap: conf_w int64[B, 4], u2, n_pos, n_neg int64[B]."""
    lib = load_evaluate_library()
    if not 1 <= int(B) <= MAX_REPLICATES:
        raise capi.HipacError(f"the bootstrap takes 1 .. {MAX_REPLICATES} replicates per call, got {B}")
    check_contract(tally.tables()["hist"])
    dev = tally.device
    with torch.cuda.device(dev):
        out = {"conf_w": torch.empty((B, 4), dtype=torch.int64, device=dev), "u2": torch.empty(B, dtype=torch.int64, device=dev),
               "n_pos": torch.empty(B, dtype=torch.int64, device=dev), "n_neg": torch.empty(B, dtype=torch.int64, device=dev)}
        capi._check(lib.hipac_evaluate_bootstrap(tally.hist.data_ptr(), tally.conf.data_ptr(), tally.G, int(seed) % 2 ** 64,
                                                 int(first_replicate), int(B), out["conf_w"].data_ptr(), out["u2"].data_ptr(),
                                                 out["n_pos"].data_ptr(), out["n_neg"].data_ptr(), capi._stream()),
                    "hipac_evaluate_bootstrap")
        return {k: v.cpu().numpy() for k, v in out.items()}


# ---- the float work (host, float64) -----------------------------------------------------------------------------------


def metrics_from_confusion(tn: int, fp: int, fn: int, tp: int) -> dict:
    """accuracy, precision, recall and f1_score as src/utils/metrics.py defines them (precision, recall and f1 are 0.0 where
    their denominator is 0), plus specificity and balanced accuracy = (recall + specificity) / 2 with the same rule.  accuracy
    is None when there are no rows (the reference's mean of an empty array is nan)."""
    tn, fp, fn, tp = int(tn), int(fp), int(fn), int(tp)
    n = tn + fp + fn + tp
    precision = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    specificity = tn / (tn + fp) if (tn + fp) > 0 else 0.0
    f1 = 2 * (precision * recall) / (precision + recall) if (precision + recall) > 0 else 0.0
    return {"accuracy": (tn + tp) / n if n else None, "precision": precision, "recall": recall, "f1_score": f1,
            "specificity": specificity, "balanced_accuracy": (recall + specificity) / 2}


def u2_of(hist_total: np.ndarray) -> int:
    """Twice the Mann-Whitney U of a [2, 4096] histogram, ties inside a bin counted half (an exact Python integer)."""
    neg, pos = [int(v) for v in hist_total[0]], [int(v) for v in hist_total[1]]
    below, u2 = 0, 0
    for b in range(len(neg)):
        u2 += pos[b] * (2 * below + neg[b])
        below += neg[b]
    return u2


def curves(hist_total) -> dict:
    """ROC, AUC and average precision of the summed histogram [2, 4096] ([true class][bin]).  A patch is called tumour at
    threshold k / 4096 when its bin is >= k.  ``thresholds`` / ``fpr`` / ``tpr``: the points at the occupied bins in descending
    order after a leading (0, 0) whose threshold is None (a rate of a missing class is None); ``auc`` = u2 / (2 n_pos n_neg),
    None for one class; ``average_precision`` = the sum over the descending occupied bins of (recall step x precision at that
    bin), None without a tumour patch."""
    h = np.asarray(hist_total, np.int64)
    if h.shape != (2, BINS):
        raise ValueError(f"curves takes the summed histogram [2, {BINS}], got {list(h.shape)}")
    neg, pos = h[0], h[1]
    n_neg, n_pos = int(neg.sum()), int(pos.sum())
    bins = np.flatnonzero(neg + pos)[::-1]
    tp, fp = np.cumsum(pos[bins]), np.cumsum(neg[bins])  # patches at or above each occupied bin
    with np.errstate(divide="ignore", invalid="ignore"):
        tpr = np.concatenate([[0], tp]) / float(n_pos)
        fpr = np.concatenate([[0], fp]) / float(n_neg)
    u2 = u2_of(h)
    auc = (float(u2) * 0.5) / (float(n_pos) * float(n_neg)) if n_pos and n_neg else None
    ap = None
    if n_pos:
        ap = 0.0
        for b, t, f in zip(bins.tolist(), tp.tolist(), fp.tolist()):  # t + f > 0: the bin is occupied
            ap += (int(pos[b]) / n_pos) * (t / (t + f))
    return {"thresholds": [None] + [b / BINS for b in bins.tolist()], "fpr": [froc_ci._num(v) for v in fpr],
            "tpr": [froc_ci._num(v) for v in tpr], "auc": auc, "average_precision": ap, "u2": u2, "n_pos": n_pos, "n_neg": n_neg}


def finish(ints: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """float64 per replicate from the integers: the five QUANTITIES, nan where a replicate does not have one -- precision
    without a positive prediction, recall without a positive label (0 / 0 both), f1 without either, auc with one class drawn.
    Where they exist they are the values ``metrics_from_confusion`` / ``curves`` give on the same integers."""
    cw = np.asarray(ints["conf_w"], np.int64)
    tn, fp, fn, tp = (cw[:, k].astype(np.float64) for k in range(4))
    n_pos, n_neg = np.asarray(ints["n_pos"], np.float64), np.asarray(ints["n_neg"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = (tn + tp) / (tn + fp + fn + tp)
        prec = np.where(tp + fp > 0, tp / (tp + fp), np.nan)
        rec = np.where(tp + fn > 0, tp / (tp + fn), np.nan)
        f1 = np.where(prec + rec > 0, 2 * (prec * rec) / (prec + rec), np.where(np.isnan(prec + rec), np.nan, 0.0))
        auc = np.where((n_pos > 0) & (n_neg > 0), (np.asarray(ints["u2"], np.float64) * 0.5) / (n_pos * n_neg), np.nan)
    return {"accuracy": acc, "precision": prec, "recall": rec, "f1_score": f1, "auc": auc}


def bootstrap_block(fin: Dict[str, np.ndarray], point: dict, B: int, seed: int, ci: float) -> dict:
    """The ``bootstrap`` entry of evaluate_<L>.json: {B, seed, ci} and one ``froc_ci.interval`` per quantity around the
    full-sample value."""
    out = {"B": int(B), "seed": int(seed), "ci": float(ci)}
    for q in QUANTITIES:
        out[q] = froc_ci.interval(point[q], fin[q], ci)
    return out


def report(names: Sequence[str], hist: np.ndarray, conf: np.ndarray, *, weights: str, level: int, balanced: bool,
           threshold: Optional[float]) -> dict:
    """The content of evaluate_<L>.json without the bootstrap, from the tables on the host."""
    tn, fp, fn, tp = (int(v) for v in conf.sum(0))
    cur = curves(hist.sum(0))
    doc = {"weights": weights, "level": int(level), "n": tn + fp + fn + tp, "class_counts": {"0": tn + fp, "1": fn + tp},
           "balanced": bool(balanced), "threshold": None if threshold is None else float(threshold),
           "confusion_matrix": [[tn, fp], [fn, tp]]}
    doc.update(metrics_from_confusion(tn, fp, fn, tp))
    doc.update({"auc": cur["auc"], "average_precision": cur["average_precision"],
                "roc": {"thresholds": cur["thresholds"], "fpr": cur["fpr"], "tpr": cur["tpr"]}, "bins": BINS})
    doc["per_slide"] = []
    for g, name in enumerate(names):
        a, b, c, d = (int(v) for v in conf[g])
        rows = a + b + c + d
        doc["per_slide"].append({"slide": name, "n": rows, "n_tumor": c + d, "TN": a, "FP": b, "FN": c, "TP": d,
                                 "accuracy": (a + d) / rows if rows else None})
    return doc


# ---- the stage ---------------------------------------------------------------------------------------------------------


def check_threshold(threshold: Optional[float]) -> Optional[float]:
    if threshold is not None and not 0.0 < float(threshold) < 1.0:
        raise ValueError(f"the decision threshold must lie strictly between 0 and 1, got {threshold}")
    return None if threshold is None else float(threshold)


def _slide_of_path(path: str) -> str:
    return os.path.basename(os.path.dirname(path))


def validation_rows(patch_dir=None, slides=None, level: int = 3, batch_size: int = 512, unbalanced: bool = False,
                    device_aug: bool = False, device="cuda"):
    """(loader, name_of, sorted slide names, row count): the validation set of ``--train`` from either of its sources, the
    loader on this rank's share of the batches, names and count over the whole set.  ``name_of(ref)`` maps one entry of a
    batch's third item (a PNG path, or a pool index) to its slide."""
    from .dist import rank_world
    from .train import get_dataloaders, get_device_loaders

    rank, world = rank_world()
    if slides is not None:
        _, loader, _, val_ds, pool = get_device_loaders(slides, level, 0.2, batch_size, rank=rank, world=world, balance_val=not unbalanced)
        row_names = [pool.slide_names[i] for i in val_ds.indices]
        return loader, (lambda ref: pool.slide_names[int(ref)]), sorted(set(row_names)), len(row_names)
    _, loader, _, val_ds = get_dataloaders(patch_dir, 0.2, batch_size, rank=rank, world=world, balance_val=not unbalanced)
    if hasattr(val_ds, "indices"):  # the balanced Subset
        paths = [val_ds.dataset.image_paths[i] for i in val_ds.indices]
    else:
        paths = list(val_ds.image_paths)
    names = sorted(set(_slide_of_path(p) for p in paths))
    if device_aug and paths:
        from .augment import OUT, DeviceClassifierLoader, DevicePatchPool

        pool = DevicePatchPool.from_patch_dataset(val_ds, device=device)
        if pool.P != OUT:
            raise EvaluateError(f"--device_aug: the patches of {patch_dir} are {pool.P} pixels; the device pool of the classifier "
                                f"loops takes {OUT}-pixel patches", 2)
        loader = DeviceClassifierLoader(pool, batch_size, shuffle=False, augment=False, rank=rank, world=world)
        return loader, (lambda ref: _slide_of_path(pool.paths[int(ref)])), names, len(paths)
    return loader, _slide_of_path, names, len(paths)


def evaluate_patches(patch_dir: Optional[str] = None, slides=None, level: int = 3, weights: str = DEFAULT_WEIGHTS,
                     precision: str = "bf16", batch_size: int = 512, threshold: Optional[float] = None, unbalanced: bool = False,
                     bootstrap: int = 0, ci: float = 95.0, seed: int = 0, device_aug: bool = False, device: str = "cuda"):
    """Score the checkpoint ``weights`` on the validation set of ``--train`` (``train.get_dataloaders(patch_dir, 0.2)[1]``, or
    ``train.get_device_loaders(slides, level, 0.2)[1]`` when ``slides`` is given: the slide-level split with random_state=42
    and the default_rng(42) class balancing ``Val Acc`` was computed on; ``unbalanced``: every patch of the validation slides).
    One ``model.predict`` per batch gives labels and logits, ``detect.tumor_probs`` the tumour probability; the decision is
    the network's argmax, or ``p > threshold`` in float32 (the reference's ``softmax_thresholding``).  A row's group is its
    slide, indexed over the sorted names of the slides in the set.  Under ``--world_size N`` every rank scores its share of
    the batches and the tables are summed over the ranks.  Returns the content of evaluate_<L>.json on rank 0, None on the
    others.  EvaluateError: rows the tally refused (status 1: a checkpoint that produces NaN must not yield a metrics file),
    a bootstrap over a single slide (status 2)."""
    from . import detect
    from .dist import rank_world
    from .resnet import ResNet18Classifier
    from .weights import canonical_state_dict, load_into

    froc_ci.check_options(bootstrap, ci)
    threshold = check_threshold(threshold)
    rank, _ = rank_world()
    dev = torch.device(device)
    loader, name_of, names, n_rows = validation_rows(patch_dir, slides, level, batch_size, unbalanced, device_aug, device)
    if not names:
        raise EvaluateError("the validation set holds no patches", 1)
    if bootstrap and len(names) < 2:
        raise EvaluateError(f"--eval_bootstrap resamples the validation slides, and there is only one ({names[0]}): no interval "
                            "can be given", 2)
    if len(names) > MAX_GROUPS:
        raise EvaluateError(f"{len(names)} validation slides: the tally takes at most {MAX_GROUPS}", 2)
    index = {n: i for i, n in enumerate(names)}
    model = ResNet18Classifier().set_precision(precision)
    load_into(model, canonical_state_dict(torch.load(weights, map_location="cpu", weights_only=True)))
    model.to(dev).eval()
    tally = PatchTally(len(names), dev)
    thr32 = None if threshold is None else float(np.float32(threshold))
    with torch.no_grad():
        for imgs, labels, refs in loader:
            pred, logits = model.predict(imgs.to(dev))
            p = detect.tumor_probs(logits.to(torch.float32).contiguous(), 1)
            decision = pred if thr32 is None else p > thr32  # float32 against the threshold rounded to float32
            group = torch.tensor([index[name_of(r)] for r in refs], dtype=torch.int32)
            tally.add(p, decision, labels, group)
    tally.all_reduce()
    if rank != 0:
        return None
    t = tally.tables()
    if t["n_bad"]:
        raise EvaluateError(f"{t['n_bad']} of {n_rows} validation patches could not be tallied (a probability that is NaN or "
                            f"outside [0, 1], or a label other than 0 and 1): '{weights}' does not score this set", 1)
    doc = report(names, t["hist"], t["conf"], weights=weights, level=level, balanced=not unbalanced, threshold=threshold)
    if bootstrap:
        fin = finish(bootstrap_integers(tally, seed, 0, bootstrap))
        doc["bootstrap"] = bootstrap_block(fin, doc, bootstrap, seed, ci)
    return doc


def bootstrap_lines(doc: dict) -> list:
    """One line per quantity of ``doc['bootstrap']``, as ``--run_evaluation --eval_bootstrap`` prints its own."""
    bs = doc["bootstrap"]
    B, ci = bs["B"], bs["ci"]
    out = []
    for q in QUANTITIES:
        e = bs[q]
        if e["lo"] is None:
            out.append(f"[INFO] patch-level {q}: undefined in all {B} replicates")
        else:
            value = "nan" if e["value"] is None else f"{e['value']:.4f}"
            out.append(f"[INFO] patch-level {q}: {value} ({ci:g} % CI {e['lo']:.4f} .. {e['hi']:.4f}; undefined in {e['undefined']} of {B} "
                       "replicates)")
    return out
