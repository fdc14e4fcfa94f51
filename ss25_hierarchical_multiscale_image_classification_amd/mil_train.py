"""Training of the ABMIL slide classifier on the device (``--train_mil`` / ``--predict_mil``).

The reference has the model (src/models/mil_classifier.py) and the bag dataset (src/datasets/mildataset.py) but never
wired a loop into its ``main.py``; ``experiments/experiment_configs.yaml`` says what the loop is (Adam, lr 1e-3, weight
decay 1e-4, 50 epochs, 32 bags per step, early stopping with patience 5, a 0.8 / 0.1 / 0.1 split, 100 patches per bag,
``models/mil_model.pth``, ``results/metrics.json``) and ``src/utils/metrics.py`` what the metrics are.

* ``NativeMILTrainer``: the parameters in one flat fp32 buffer (``train_native.FlatAdam``); one step = one
  ``hipac_mil_train_fwd_bwd`` (include/hipac_mil_train.h, ``csrc/mil_train.hip``) over a batch of ragged bags that are
  rows of the resident feature matrix, the L2 term, ``hipac_adam_step``.
* ``train_mil`` / ``predict_mil``: the loop and the scoring over the (features, labels, paths) triple that
  ``--extract_features`` writes.  Validation and prediction go through ``MILClassifier.forward_bags``.
* Multi-head attention pooling (the yaml's ``attention_heads``, ``--mil_heads K``) comes from ``mil_heads.py``: a model
  whose ``aggregator.attn_U.weight`` has K > 1 rows trains through ``hipac_mil_heads_train_fwd_bwd`` and is scored through
  ``hipac_mil_heads_forward``; one head goes the way it always went.
* Gated attention (Ilse et al. 2018, eq. 9; ``--mil_gated``) comes from ``mil_gated.py``: a model with the
  ``aggregator.attn_G`` keys trains through ``hipac_mil_gated_train_fwd_bwd`` and is scored through
  ``hipac_mil_gated_forward``, for any head count; an ungated model takes exactly the calls it always took.
* Multiscale bags (``--mil_levels 1,2,3``) come from ``mil_levels.py``: a model with the ``aggregator.levels`` buffer trains
  through ``hipac_mil_levels_train_fwd_bwd`` and is scored through ``hipac_mil_levels_forward`` over the triples of all its
  levels, with one attention branch and one softmax per level; any other model takes exactly the calls it always took.
* Dropout (the yaml's ``dropout_rate``) and Monte-Carlo dropout uncertainty (its ``uncertainty_estimation``) come from
  ``mil_dropout.py``: the trainer's step under ``hipac_mil_dropout_train_fwd_bwd``, ``predict_mil``'s
  ``results/mil_uncertainty.csv`` from ``mil_dropout.mc_forward``.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi, mil_dropout, mil_gated, mil_heads, mil_levels
from .mil import MILClassifier, group_patches_by_wsi
from .train_native import FlatAdam

MIL_TRAIN_ABI_VERSION = 1  # include/hipac_mil_train.h HIPAC_MIL_TRAIN_ABI_VERSION this binding was written against

# name -> (restype, argtypes); must list every symbol include/hipac_mil_train.h declares (tests/test_mil_train_capi_symbols.py)
MIL_TRAIN_SYMBOLS = {
    "hipac_mil_train_abi_version": (C.c_int, []),
    "hipac_mil_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_train_fwd_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_int, C.c_void_p]),
    "hipac_mil_train_l2_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
}

_bound = None


def load_mil_train_library():
    """The library of ``capi.load_library()`` with the MIL training entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, MIL_TRAIN_SYMBOLS, "hipac_mil_train_abi_version", MIL_TRAIN_ABI_VERSION,
                                   "MIL training ABI")
    return lib


# state_dict key -> hipac_mil_params_t field, in the order of the flat buffer
PARAM_FIELDS = (("aggregator.attn_V.weight", "attn_V_w"), ("aggregator.attn_V.bias", "attn_V_b"),
                ("aggregator.attn_U.weight", "attn_U_w"), ("aggregator.attn_U.bias", "attn_U_b"),
                ("classifier.0.weight", "fc1_w"), ("classifier.0.bias", "fc1_b"),
                ("classifier.2.weight", "fc2_w"), ("classifier.2.bias", "fc2_b"))
# the gate of a gated model (hipac_mil_gated_params_t's own fields): in the flat buffer after aggregator.attn_U.bias
GATE_FIELDS = ((mil_gated.GATE_W, "attn_G_w"), (mil_gated.GATE_B, "attn_G_b"))


class NativeMILTrainer:
    """``MILClassifier`` under torch.optim.Adam(lr, weight_decay) with the whole step in HIP.  ``sd``: a MILClassifier
    state_dict (any device, converted to float32); the parameters live in one flat buffer, every tensor starting on a
    16-byte boundary (the gaps stay 0).  ``dropout`` > 0: every forward_backward runs under the masks of
    (``seed``, sample = the number of steps taken so far) -- include/hipac_mil_dropout.h; 0 is the step as it always was.
    The head count is the number of rows of ``aggregator.attn_U.weight``: more than one runs
    ``hipac_mil_heads_train_fwd_bwd`` (include/hipac_mil_heads.h; not under dropout), one ``hipac_mil_train_fwd_bwd``.
    A state_dict with the ``aggregator.attn_G`` keys (attention pooling) is a gated model: it runs
    ``hipac_mil_gated_train_fwd_bwd`` (include/hipac_mil_gated.h; not under dropout) for any head count, the two gate
    tensors live in the same flat buffer (so Adam and the L2 term cover them) and ``self.attn`` is [n, heads].
    A state_dict with the ``aggregator.levels`` buffer (attention pooling, ungated, no dropout) is a levels model: it runs
    ``hipac_mil_levels_train_fwd_bwd`` (include/hipac_mil_levels.h), ``forward_backward`` / ``step`` then need ``level_of``,
    ``self.attn`` is [n], and ``state_dict`` carries the buffer along."""

    def __init__(self, sd: Dict[str, torch.Tensor], pooling: str, device, lr: float = 1e-3, weight_decay: float = 1e-4,
                 class_weights=None, dropout: float = 0.0, seed: int = 0):
        if pooling not in capi.MIL_POOLING:
            raise ValueError("Unknown pooling: choose from 'attention', 'mean', 'max'")
        self.keys = [k for k, _ in PARAM_FIELDS if pooling == "attention" or not k.startswith("aggregator.")]
        self.gated = pooling == "attention" and mil_gated.is_gated(sd)
        if self.gated:  # the model's own key order: the gate follows aggregator.attn_U
            at = self.keys.index("aggregator.attn_U.bias") + 1
            self.keys[at:at] = [k for k, _ in GATE_FIELDS]
        missing = [k for k in self.keys if k not in sd]
        if missing:
            raise capi.HipacError(f"state_dict lacks {missing}")
        self.heads = mil_heads.model_dims(sd, pooling)[0]  # ValueError if classifier.0.weight disagrees with heads * feature_dim
        self.levels = mil_levels.model_levels(sd) if pooling == "attention" else None  # ValueError if it disagrees with attn_U
        self.dropout, self.seed, self.steps = mil_dropout.check_p(dropout), int(seed) & 0xFFFFFFFFFFFFFFFF, 0
        if self.levels is not None and (self.gated or self.dropout > 0.0):
            raise ValueError("a levels model is ungated and trains without dropout: every level has one plain attention branch")
        if self.heads > 1 and self.dropout > 0.0:
            raise ValueError("dropout with more than one attention head is not implemented: the masked step is single-head")
        if self.gated and self.dropout > 0.0:
            raise ValueError("dropout with gated attention is not implemented: the masked step is single-head and ungated")
        if self.gated:
            mil_gated.gated_dims(sd)  # ValueError if the gate's shapes disagree with attn_V, before anything is loaded
        self.lib = load_mil_train_library()
        # the step's entry point, decided once: (workspace query, step, the int after the params -- heads / levels / pooling --,
        # the arguments that follow `accumulate`, whether attn is [n] and not [n, heads])
        if self.gated:
            mil_gated.load_mil_gated_library()
            self._entry = ("hipac_mil_gated_train_workspace_bytes", "hipac_mil_gated_train_fwd_bwd", self.heads, lambda: (), False)
        elif self.levels is not None:
            mil_levels.load_mil_levels_library()
            self._entry = ("hipac_mil_levels_train_workspace_bytes", "hipac_mil_levels_train_fwd_bwd", self.heads, lambda: (), True)
        elif self.heads > 1:
            mil_heads.load_mil_heads_library()
            self._entry = ("hipac_mil_heads_train_workspace_bytes", "hipac_mil_heads_train_fwd_bwd", self.heads, lambda: (), False)
        elif self.dropout > 0.0:
            mil_dropout.load_mil_dropout_library()
            self._entry = ("hipac_mil_dropout_train_workspace_bytes", "hipac_mil_dropout_train_fwd_bwd", capi.MIL_POOLING[pooling],
                           lambda: (self.dropout, self.seed, self.steps & 0xFFFFFFFF), True)
        else:
            self._entry = ("hipac_mil_train_workspace_bytes", "hipac_mil_train_fwd_bwd", capi.MIL_POOLING[pooling], lambda: (), True)
        self.pooling, self.device, self.weight_decay = pooling, torch.device(device), float(weight_decay)
        if self.device.type != "cuda":
            raise capi.HipacError("NativeMILTrainer needs a ROCm device: there is no CPU fallback")
        self.shapes = {k: tuple(sd[k].shape) for k in self.keys}
        self.offsets, o = {}, 0
        for k in self.keys:
            self.offsets[k] = o
            o += (int(np.prod(self.shapes[k])) + 3) // 4 * 4
        self.opt = FlatAdam(o, self.device, lr)
        for k in self.keys:
            self._view(self.opt.params, k).copy_(sd[k].detach().to(self.device, torch.float32))
        self.F, self.hidden = int(self.shapes["classifier.0.weight"][1]) // self.heads, int(self.shapes["classifier.0.weight"][0])
        self.C = int(self.shapes["classifier.2.weight"][0])
        self.A = int(self.shapes["aggregator.attn_V.weight"][0]) if pooling == "attention" else 0
        if pooling == "attention" and self.shapes["aggregator.attn_V.weight"] != (self.A, self.F):
            raise capi.HipacError("aggregator.attn_V.weight does not match feature_dim")
        if pooling == "attention" and (self.shapes["aggregator.attn_U.weight"] != (self.heads, self.A) or
                                       self.shapes["aggregator.attn_U.bias"] != (self.heads,)):
            raise capi.HipacError("aggregator.attn_U does not match aggregator.attn_V")
        if self.shapes["classifier.2.weight"] != (self.C, self.hidden):
            raise capi.HipacError("classifier.2.weight does not match classifier.0.weight")
        self._p, self._g = self._struct(self.opt.params), self._struct(self.opt.grads)
        self.class_weights = None if class_weights is None else \
            torch.as_tensor(class_weights, dtype=torch.float32).to(self.device).contiguous()
        if self.class_weights is not None and self.class_weights.numel() != self.C:
            raise capi.HipacError(f"class_weights must have {self.C} entries")
        self._ws: Optional[torch.Tensor] = None
        self.attn: Optional[torch.Tensor] = None

    def _view(self, flat: torch.Tensor, key: str) -> torch.Tensor:
        o = self.offsets[key]
        return flat[o:o + int(np.prod(self.shapes[key]))].view(self.shapes[key])

    def _struct(self, flat: torch.Tensor):
        """hipac_mil_params_t over the flat buffer; hipac_mil_gated_params_t (which starts with one) for a gated model."""
        out = mil_gated.MilGatedParams() if self.gated else capi.MilParams()
        p = out.base if self.gated else out
        for k, field in PARAM_FIELDS:
            if k in self.offsets:
                setattr(p, field, flat.data_ptr() + 4 * self.offsets[k])
        p.feature_dim, p.attn_dim, p.hidden_dim, p.num_classes = self.F, self.A, self.hidden, self.C
        if self.gated:
            for k, field in GATE_FIELDS:
                setattr(out, field, flat.data_ptr() + 4 * self.offsets[k])
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's key names; loads into its MILClassifier and into ``mil.MILClassifier`` with strict=True."""
        out = {k: self._view(self.opt.params, k).clone() for k in self.keys}
        if self.levels is not None:
            out[mil_levels.LEVELS_KEY] = torch.tensor(self.levels, dtype=torch.int64, device=self.device)
        return out

    def grad_dict(self) -> Dict[str, torch.Tensor]:
        return {k: self._view(self.opt.grads, k).clone() for k in self.keys}

    def forward_backward(self, feats: torch.Tensor, rows, offsets, labels, accumulate: bool = False, want_attn: bool = False,
                         level_of=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """feats float32[N, F] on the device (stays in place); rows int[n] indices into it, or None for
        the identity (then offsets must end at N); offsets int[n_bags + 1]; labels int64[n_bags] -> (loss float32[], logits[n_bags, C]);
        the gradients land in the flat buffer (``grad_dict``); ``want_attn`` keeps the softmax weights in ``self.attn``
        ([n], or [n, heads] for more than one head and for a gated model).  ``level_of`` int[n]: the level slot of every BATCH
        row, for a levels model and only for one (ValueError otherwise); ``self.attn`` is then [n].  Everything is checked on
        the host before the launch: a bad row index never reaches a kernel."""
        if (level_of is not None) != (self.levels is not None):
            raise ValueError("level_of goes with a levels model (one with aggregator.levels), and such a model needs it")
        if not torch.is_tensor(feats) or not feats.is_cuda:
            raise capi.HipacError("HIP path called with a CPU tensor: there is no CPU fallback (move inputs to cuda)")
        if feats.dtype != torch.float32 or feats.dim() != 2 or not feats.is_contiguous() or feats.device != self.device:
            raise capi.HipacError(f"feats must be a contiguous float32[N, feature_dim] tensor on {self.device}")
        N, F = int(feats.shape[0]), int(feats.shape[1])
        if F != self.F:
            raise capi.HipacError(f"feats has {F} columns, the model {self.F}")
        offs = np.asarray(offsets.detach().cpu() if torch.is_tensor(offsets) else offsets).astype(np.int64).ravel()
        if offs.size < 2 or offs[0] != 0 or bool((offs[1:] <= offs[:-1]).any()):
            raise capi.HipacError("offsets must start at 0 and increase strictly (no empty bags)")
        n, n_bags = int(offs[-1]), offs.size - 1
        if rows is None:
            if n > N:
                raise capi.HipacError(f"offsets cover {n} rows, feats has {N}")
            if n != N:
                raise capi.HipacError(f"offsets must end at the number of rows ({N}), got {n}")
            rows_dev = None
        else:
            r = torch.as_tensor(rows)
            if r.dim() != 1 or r.dtype not in (torch.int32, torch.int64):
                raise capi.HipacError("rows must be a 1-d int32 / int64 index")
            if int(r.numel()) != n:
                raise capi.HipacError(f"offsets must end at the number of rows ({int(r.numel())}), got {n}")
            if n and (int(r.min()) < 0 or int(r.max()) >= N):
                raise capi.HipacError(f"rows holds an index outside [0, {N})")
            rows_dev = r.to(self.device, torch.int32).contiguous()
        lab = torch.as_tensor(labels)
        if lab.dim() != 1 or int(lab.numel()) != n_bags or lab.dtype != torch.int64:
            raise capi.HipacError(f"labels must be int64[{n_bags}]")
        if n_bags and (int(lab.min()) < 0 or int(lab.max()) >= self.C):
            raise capi.HipacError(f"labels holds a class outside [0, {self.C})")
        lab = lab.to(self.device).contiguous()
        offs_dev = torch.from_numpy(offs.astype(np.int32)).to(self.device)
        lv_dev = None if level_of is None else mil_levels._check_level_of(level_of, n).to(self.device, torch.uint8).contiguous()
        query_name, step_name, first, extra, attn_1d = self._entry
        need = getattr(self.lib, query_name)(C.addressof(self._p), first, n, n_bags)
        if need == 0:
            raise capi.HipacError(f"mil training step of {n} rows in {n_bags} bags refused (sizes outside the kernel's limits)")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        logits = torch.empty((n_bags, self.C), dtype=torch.float32, device=self.device)
        self.attn = torch.empty(n if attn_1d else (n, self.heads), dtype=torch.float32, device=self.device) \
            if (want_attn and self.pooling == "attention") else None
        level = () if lv_dev is None else (lv_dev.data_ptr(),)  # level_of goes in after rows
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, step_name)(
                C.addressof(self._p), first, feats.data_ptr(), N, capi._ptr(rows_dev), *level, offs_dev.data_ptr(), n, n_bags,
                lab.data_ptr(), capi._ptr(self.class_weights), C.addressof(self._g), loss.data_ptr(), logits.data_ptr(),
                capi._ptr(self.attn), self._ws.data_ptr(), self._ws.numel(), 1 if accumulate else 0, *extra(), capi._stream())
        capi._check(rc, step_name)
        return loss, logits

    def step(self, feats, rows, offsets, labels, level_of=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """forward_backward, the L2 term (g += weight_decay * p, torch-Adam's form), one Adam update."""
        loss, logits = self.forward_backward(feats, rows, offsets, labels, level_of=level_of)
        if self.weight_decay != 0.0:
            with torch.cuda.device(self.device):
                capi._check(self.lib.hipac_mil_train_l2_add(self.opt.grads.data_ptr(), self.opt.params.data_ptr(),
                                                            self.opt.params.numel(), self.weight_decay, capi._stream()),
                            "hipac_mil_train_l2_add")
        self.opt.step()
        self.steps += 1
        return loss, logits


# ----------------------------------------------------------------------------
# host side of the loop: split, epoch batches, metrics
# ----------------------------------------------------------------------------
def split_bags(n_bags: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A seeded permutation of the bags cut 0.8 / 0.1 / 0.1 -> (train, val, test) bag indices.  Train gets at least one
    bag; val and test get int(0.1 n) each (so both are empty below 10 bags) and train the rest."""
    if n_bags < 1:
        raise ValueError("no bags to split")
    perm = np.random.default_rng(seed).permutation(n_bags)
    n_val = n_test = int(0.1 * n_bags)
    n_train = n_bags - n_val - n_test
    return perm[:n_train], perm[n_train:n_train + n_val], perm[n_train + n_val:]


def epoch_batches(train_bags: Sequence[int], order: np.ndarray, offsets: np.ndarray, epoch: int, seed: int = 0,
                  bags_per_step: int = 32, bag_size: Optional[int] = None):
    """The steps of one epoch: a seeded shuffle of the training bags, cut into groups of ``bags_per_step``; with
    ``bag_size`` a seeded sample without replacement of at most that many rows of each bag (in the bag's own order).
    Yields (rows int32[n] into the feature matrix, offsets int64[k + 1], bag indices int64[k]).  A function of
    (seed, epoch) only."""
    rng = np.random.default_rng([seed, epoch + 1])
    bags = np.asarray(train_bags, np.int64)[rng.permutation(len(train_bags))]
    for s in range(0, len(bags), bags_per_step):
        group = bags[s:s + bags_per_step]
        rows, offs = [], [0]
        for b in group:
            r = order[offsets[b]:offsets[b + 1]]
            if bag_size is not None and len(r) > bag_size:
                r = r[np.sort(rng.choice(len(r), size=bag_size, replace=False))]
            rows.append(r)
            offs.append(offs[-1] + len(r))
        yield np.concatenate(rows).astype(np.int32), np.asarray(offs, np.int64), group


def classification_metrics(y_true, y_pred) -> Dict[str, object]:
    """src/utils/metrics.py: accuracy, precision / recall / F1 of class 1 (0.0 where a denominator is 0) and the
    confusion matrix, as plain Python numbers."""
    t, p = np.asarray(y_true).astype(np.int64).ravel(), np.asarray(y_pred).astype(np.int64).ravel()
    tp, tn = int(((t == 1) & (p == 1)).sum()), int(((t == 0) & (p == 0)).sum())
    fp, fn = int(((t == 0) & (p == 1)).sum()), int(((t == 1) & (p == 0)).sum())
    prec = tp / (tp + fp) if tp + fp > 0 else 0.0
    rec = tp / (tp + fn) if tp + fn > 0 else 0.0
    return {"accuracy": float((t == p).mean()) if t.size else 0.0, "precision": float(prec), "recall": float(rec),
            "f1_score": float(2 * prec * rec / (prec + rec)) if prec + rec > 0 else 0.0,
            "confusion_matrix": {"TP": tp, "TN": tn, "FP": fp, "FN": fn}}


def load_triple(features_path, labels_path, paths_path, by_slide: bool = False):
    """-> (features float32[N, F], order, offsets, bag names, bag labels) of the files ``--extract_features`` writes."""
    feats = np.load(features_path)
    labels = np.load(labels_path)
    with open(paths_path, "r") as f:
        paths = [line.strip() for line in f if line.strip()]
    if feats.ndim != 2 or len(paths) != feats.shape[0] or labels.shape[0] != feats.shape[0]:
        raise ValueError(f"triple does not agree: features {feats.shape}, labels {labels.shape}, {len(paths)} paths")
    order, offsets, names, wsi = group_patches_by_wsi(paths, labels, by_slide)
    return np.ascontiguousarray(feats, dtype=np.float32), order, offsets, names, wsi


def initial_state_dict(feature_dim: int, pooling: str, seed: int, heads: int = 1, gated: bool = False, levels=None
                       ) -> Dict[str, torch.Tensor]:
    """MILClassifier's own (torch default) initialisation under ``torch.manual_seed(seed)``, drawn on the CPU.  The gate of a
    gated model is drawn after ``attn_V`` and ``attn_U``.  ``levels``: a levels model, with its ``aggregator.levels`` buffer."""
    gen_state = torch.get_rng_state()
    torch.manual_seed(seed)
    try:
        return {k: v.detach().clone() for k, v in MILClassifier(feature_dim, 2, pooling, heads=heads, gated=gated,
                                                                  levels=levels).state_dict().items()}
    finally:
        torch.set_rng_state(gen_state)


def _gathered(feats_dev: torch.Tensor, bags, order, offsets):
    """Contiguous copy of the rows of ``bags`` (made once for the val / test split: forward_bags wants bag rows contiguous)."""
    rows = np.concatenate([order[offsets[b]:offsets[b + 1]] for b in bags])
    offs = np.concatenate([[0], np.cumsum([offsets[b + 1] - offsets[b] for b in bags])]).astype(np.int64)
    return feats_dev[torch.from_numpy(rows).to(feats_dev.device)].contiguous(), offs


def _gathered_levels(level_rows: np.ndarray, bags, order, offsets) -> np.ndarray:
    """The level slots of the rows ``_gathered`` copies, in its order."""
    return np.ascontiguousarray(level_rows[np.concatenate([order[offsets[b]:offsets[b + 1]] for b in bags])], dtype=np.uint8)


def _score(sd, pooling, feats: torch.Tensor, offs: np.ndarray, want_attn: bool = False, level_of=None):
    """The logits of the bags under the model ``sd`` (its head count and its gate read from the state_dict); with
    ``want_attn`` also the attention [n, heads] (None for mean / max pooling).  ``level_of``: the level slots of the rows, for a
    levels model (one with ``aggregator.levels``) and only for one; its attention is [n, 1]."""
    if level_of is not None:
        model = MILClassifier(feats.shape[1], int(sd["classifier.2.weight"].shape[0]), pooling,
                              levels=mil_levels.model_levels(sd)).to(feats.device)
        model.load_state_dict(sd, strict=True)
        model.eval()
        logits, attn = model.forward_bags(feats, offs, level_of=level_of)
        return (logits, attn.reshape(feats.shape[0], 1)) if want_attn else logits
    heads = mil_heads.model_dims(sd, pooling)[0]
    gated = pooling == "attention" and mil_gated.is_gated(sd)
    model = MILClassifier(feats.shape[1], int(sd["classifier.2.weight"].shape[0]), pooling, heads=heads, gated=gated).to(feats.device)
    model.load_state_dict(sd, strict=True)
    model.eval()
    logits, attn = model.forward_bags(feats, offs)
    if not want_attn:
        return logits
    return logits, (None if attn is None else attn.reshape(feats.shape[0], heads))


def train_mil(features_path, labels_path, paths_path, *, pooling: str = "attention", by_slide: bool = False, epochs: int = 50,
              bags_per_step: int = 32, bag_size: Optional[int] = None, lr: float = 1e-3, weight_decay: float = 1e-4,
              patience: int = 5, seed: int = 0, out_dir: str = ".", max_steps: Optional[int] = None, device=None,
              dropout: float = 0.0, heads: int = 1, gated: bool = False, levels=None, data_dir: str = ".") -> Dict[str, object]:
    """The yaml's loop (module docstring).  Writes ``<out_dir>/models/mil_model.pth`` (the state with the best validation
    loss; the last one when there is no validation split) and ``<out_dir>/results/metrics.json``; returns the metrics.
    ``dropout`` > 0 trains under dropout (masks seeded by ``seed``); validation and test scoring stay deterministic, and
    the metrics then carry a ``"dropout"`` key.  ``heads`` > 1 (attention pooling, no dropout) trains the multi-head model
    and the metrics carry ``"attention_heads"``.  ``gated`` (attention pooling, no dropout, any ``heads``) trains the gated
    model and the metrics carry ``"gated_attention": true``.  ``levels`` (two or more pyramid levels, ascending; attention
    pooling, one head, ungated, no dropout) trains the multiscale model of ``mil_levels.py``: the three paths are not read
    (give None), the bags are those of ``mil_levels.load_triples(levels, data_dir)`` (one per slide, whatever ``by_slide``
    says), ``bag_size`` samples per (bag, level), and the metrics carry ``"levels"``."""
    dropout, heads, gated = mil_dropout.check_p(dropout), mil_heads.check_heads(heads), bool(gated)
    if levels is not None:
        levels = mil_levels.check_levels(levels)
        if pooling != "attention" or heads > 1 or gated or dropout > 0.0:
            raise ValueError("levels needs attention pooling with one head per level, ungated and without dropout")
    if heads > 1 and pooling != "attention":
        raise ValueError(f"heads = {heads} needs attention pooling, not {pooling}")
    if heads > 1 and dropout > 0.0:
        raise ValueError("dropout with more than one attention head is not implemented: the masked step is single-head")
    if gated and pooling != "attention":
        raise ValueError(f"gated attention needs attention pooling, not {pooling}")
    if gated and dropout > 0.0:
        raise ValueError("dropout with gated attention is not implemented: the masked step is single-head and ungated")
    if levels is None:
        feats, order, offsets, names, wsi = load_triple(features_path, labels_path, paths_path, by_slide)
        level_rows = None
    else:
        feats, level_rows, order, offsets, names, wsi, _ = mil_levels.load_triples(levels, data_dir)
    lv = (lambda bags: {}) if levels is None else (lambda bags: {"level_of": _gathered_levels(level_rows, bags, order, offsets)})
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    tr, va, te = split_bags(len(names), seed)
    print(f"[INFO] MIL: {len(names)} bags of {feats.shape[0]} patches; train / val / test = {len(tr)} / {len(va)} / {len(te)}")
    if len(va) == 0:
        print("[INFO] MIL: the validation split is empty: early stopping is off")
    feats_dev = torch.from_numpy(feats).to(dev)  # uploaded once; every step reads it in place through a row index
    trainer = NativeMILTrainer(initial_state_dict(feats.shape[1], pooling, seed, heads, gated, levels), pooling, dev, lr=lr,
                               weight_decay=weight_decay, dropout=dropout, seed=seed)
    labels_all = torch.from_numpy(wsi)
    val = _gathered(feats_dev, va, order, offsets) if len(va) else None
    val_labels = labels_all[torch.from_numpy(va)].to(dev) if len(va) else None
    val_lv = lv(va) if len(va) else {}
    history = {"train_loss": [], "val_loss": []}
    best, best_sd, bad, steps, stopped = float("inf"), None, 0, 0, False
    for epoch in range(epochs):
        losses = []
        batches = epoch_batches(tr, order, offsets, epoch, seed, bags_per_step, bag_size) if levels is None else \
            mil_levels.epoch_batches(tr, order, offsets, level_rows, len(levels), epoch, seed, bags_per_step, bag_size)
        for rows, offs, group, *batch_lv in batches:  # a levels batch carries the level slots of its rows
            loss, _ = trainer.step(feats_dev, rows, offs, labels_all[torch.from_numpy(group)], *batch_lv)
            losses.append(loss)
            steps += 1
            if max_steps is not None and steps >= max_steps:
                break
        history["train_loss"].append(float(torch.stack(losses).mean().item()))
        msg = f"[INFO] MIL epoch {epoch + 1}/{epochs}: train loss {history['train_loss'][-1]:.6f}"
        if val is not None:
            v = float(torch.nn.functional.cross_entropy(_score(trainer.state_dict(), pooling, *val, **val_lv), val_labels).item())
            history["val_loss"].append(v)
            msg += f", val loss {v:.6f}"
            if v < best:
                best, best_sd, bad = v, trainer.state_dict(), 0
            else:
                bad += 1
        print(msg)
        if max_steps is not None and steps >= max_steps:
            break
        if val is not None and bad >= patience:
            print(f"[INFO] MIL: early stopping after epoch {epoch + 1} (no better validation loss for {patience} epochs)")
            stopped = True
            break
    if best_sd is None:
        best_sd = trainer.state_dict()
    os.makedirs(os.path.join(out_dir, "models"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "results"), exist_ok=True)
    model_path = os.path.join(out_dir, "models", "mil_model.pth")
    torch.save({k: v.cpu() for k, v in best_sd.items()}, model_path)
    if len(te):
        tf, toffs = _gathered(feats_dev, te, order, offsets)
        pred = _score(best_sd, pooling, tf, toffs, **lv(te)).argmax(1).cpu().numpy()
        metrics = classification_metrics(wsi[te], pred)
    else:
        print("[INFO] MIL: the test split is empty: the metrics are those of no predictions")
        metrics = classification_metrics([], [])
    metrics.update({"train_loss": history["train_loss"], "val_loss": history["val_loss"], "epochs_run": len(history["train_loss"]),
                    "steps": steps, "early_stopped": stopped, "pooling": pooling,
                    "split_sizes": {"train": int(len(tr)), "val": int(len(va)), "test": int(len(te))}})
    if dropout > 0.0:
        metrics["dropout"] = dropout
    if heads > 1:
        metrics["attention_heads"] = heads
    if gated:
        metrics["gated_attention"] = True
    if levels is not None:
        metrics["levels"] = [int(v) for v in levels]
    with open(os.path.join(out_dir, "results", "metrics.json"), "w") as f:
        json.dump(metrics, f, indent=2)
    print(f"[INFO] MIL: model saved to {model_path}; test accuracy {metrics['accuracy']:.4f}")
    return metrics


def predict_mil(model_path, features_path, labels_path, paths_path, *, pooling: str = "attention", by_slide: bool = False,
                out_dir: str = ".", device=None, dropout: float = 0.0, mc_samples: int = 0, threshold: float = 0.5, seed: int = 0,
                heads: Optional[int] = None, save_attention: bool = False, levels=None, data_dir: str = "."
                ) -> List[Tuple[str, float, int]]:
    """Every bag of the triple scored with a saved model -> [(bag name, probability of class 1, predicted label)], also
    written as ``<out_dir>/results/mil_predictions.csv``.  With ``mc_samples`` > 0 (needs ``dropout`` > 0) it also writes
    ``<out_dir>/results/mil_uncertainty.csv``: per bag the mean and the variance (divisor T - 1, ``torch.var``) of the
    class-1 probability over ``mc_samples`` stochastic forwards, the entropy of the mean, the mean entropy, their difference
    (the mutual information), and ``mean_probability > threshold`` (the reference's ``softmax_thresholding``).
    The head count is the saved model's; ``heads``, when given, must agree with it.  A gated model (one saved with the
    ``aggregator.attn_G`` keys) is recognised as such; it has no Monte-Carlo dropout pass.  ``save_attention`` (attention pooling)
    also writes ``<out_dir>/results/mil_attention.npy``: float32 [n, heads], row i the softmax weights of the patch on line
    i of the paths file inside its bag -- what the reference's src/visualization/attention_heatmap.py takes.
    A levels model (one saved with the ``aggregator.levels`` buffer) is scored with ``features_path`` = None: the triples of
    the model's own levels are read from ``data_dir`` (``mil_levels.load_triples``), one bag per slide; ``levels``, when given,
    must agree with the model.  ``save_attention`` then writes ``<out_dir>/results/mil_attention_<L>.npy`` per level, float32
    [patches_L, 1], row i the weight of the patch on line i of ``patch_paths_<L>.txt`` inside its (slide, level)."""
    dropout, mc_samples = mil_dropout.check_p(dropout), int(mc_samples)
    if mc_samples < 0 or mc_samples > mil_dropout.MC_MAX_SAMPLES:
        raise ValueError(f"mc_samples must be in 0..{mil_dropout.MC_MAX_SAMPLES}, got {mc_samples}")
    if mc_samples > 0 and dropout == 0.0:
        raise ValueError("Monte-Carlo dropout needs a dropout probability: give --mil_dropout P with 0 < P < 1 "
                         "(with P = 0 every sample is the same forward)")
    multiscale = features_path is None
    if multiscale:
        model_lv = mil_levels.model_levels(torch.load(model_path, map_location="cpu", weights_only=True)) if pooling == "attention" else None
        if model_lv is None:
            raise ValueError(f"{model_path} is not a levels model: give the triple of one level")
        if levels is not None and tuple(int(v) for v in levels) != model_lv:
            raise ValueError(f"levels = {','.join(str(int(v)) for v in levels)}, but {model_path} was trained on levels "
                             f"{','.join(map(str, model_lv))}")
        if dropout > 0.0 or mc_samples > 0:
            raise ValueError("Monte-Carlo dropout with a levels model is not implemented: the fused pass is single-scale")
        feats, level_rows, order, offsets, names, _, starts = mil_levels.load_triples(model_lv, data_dir)
    else:
        feats, order, offsets, names, _ = load_triple(features_path, labels_path, paths_path, by_slide)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    sd = {k: v.to(dev, torch.int64 if k == mil_levels.LEVELS_KEY else torch.float32).contiguous()
          for k, v in torch.load(model_path, map_location="cpu", weights_only=True).items()}
    if not multiscale and (levels is not None or mil_levels.LEVELS_KEY in sd):
        raise ValueError(f"{model_path} is a levels model: it is scored over the triples of its own levels, not over one triple"
                         if mil_levels.LEVELS_KEY in sd else f"levels given, but {model_path} is not a levels model")
    model_heads = mil_heads.model_dims(sd, pooling)[0]
    if heads is not None and mil_heads.check_heads(heads) != model_heads:
        raise ValueError(f"heads = {heads}, but {model_path} has {model_heads} attention head(s)")
    if model_heads > 1 and (dropout > 0.0 or mc_samples > 0):
        raise ValueError("Monte-Carlo dropout with more than one attention head is not implemented: the fused pass is single-head")
    if pooling == "attention" and mil_gated.is_gated(sd) and (dropout > 0.0 or mc_samples > 0):
        raise ValueError("Monte-Carlo dropout with gated attention is not implemented: the fused pass is single-head and ungated")
    if save_attention and pooling != "attention":
        raise ValueError(f"save_attention needs attention pooling: {pooling} pooling has no attention weights")
    feats_dev = torch.from_numpy(feats).to(dev)
    f, offs = _gathered(feats_dev, np.arange(len(names)), order, offsets)
    score_lv = {"level_of": _gathered_levels(level_rows, np.arange(len(names)), order, offsets)} if multiscale else {}
    logits, attn = _score(sd, pooling, f, offs, want_attn=True, **score_lv)
    prob = torch.softmax(logits, dim=1)[:, 1].cpu().numpy()
    pred = logits.argmax(1).cpu().numpy()
    out = [(n, float(p), int(y)) for n, p, y in zip(names, prob, pred)]
    os.makedirs(os.path.join(out_dir, "results"), exist_ok=True)
    with open(os.path.join(out_dir, "results", "mil_predictions.csv"), "w") as fh:
        fh.write("bag,probability,prediction\n")
        for n, p, y in out:
            fh.write(f"{n},{p:.6f},{y}\n")
    print(f"[INFO] MIL: {len(out)} bags scored -> {os.path.join(out_dir, 'results', 'mil_predictions.csv')}")
    if save_attention and multiscale:
        for level, table in zip(model_lv, mil_levels.attention_tables(attn.cpu().numpy(), order, starts)):
            path = os.path.join(out_dir, "results", f"mil_attention_{level}.npy")
            np.save(path, table)
            print(f"[INFO] MIL: attention of level {level} over {table.shape[0]} patches -> {path}")
    elif save_attention:
        table = np.empty((feats.shape[0], model_heads), np.float32)
        table[order] = attn.cpu().numpy()  # gathered row i is line order[i] of the paths file
        path = os.path.join(out_dir, "results", "mil_attention.npy")
        np.save(path, table)
        print(f"[INFO] MIL: attention of {model_heads} head(s) over {feats.shape[0]} patches -> {path}")
    if mc_samples > 0:
        if int(sd["classifier.2.weight"].shape[0]) < 2:
            raise ValueError("the uncertainty table reports class 1: the model needs at least two classes")
        mc = mil_dropout.mc_forward(sd, pooling, f, offs, dropout, seed, mc_samples)
        cols = [mc["mean_prob"][:, 1], mc["var_prob"][:, 1], mc["entropy"], mc["expected_entropy"], mc["mutual_info"]]
        table = torch.stack(cols, dim=1).cpu().numpy()
        path = os.path.join(out_dir, "results", "mil_uncertainty.csv")
        with open(path, "w") as fh:
            fh.write("bag,mean_probability,variance,entropy,expected_entropy,mutual_information,prediction\n")
            for name, row in zip(names, table):
                fh.write(f"{name},{row[0]:.6f},{row[1]:.6e},{row[2]:.6f},{row[3]:.6f},{row[4]:.6f},{int(row[0] > threshold)}\n")
        print(f"[INFO] MIL: {mc_samples} Monte-Carlo dropout samples (p = {dropout}) -> {path}")
    return out
