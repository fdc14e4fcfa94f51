"""Multiscale MIL bags with per-level attention (``--mil_levels 1,2,3``): the ctypes binding of include/hipac_mil_levels.h
(``csrc/mil_levels.hip``) and the bag building over several pyramid levels.

A slide's bag holds the feature rows of all chosen levels.  Every level has its own attention branch over the shared hidden
layer (``aggregator.attn_U`` is ``Linear(attn_dim, L)``) and its own softmax over that level's rows of the slide; the L pooled
vectors are concatenated level-major and ``classifier.0`` is ``Linear(L * feature_dim, hidden)`` -- the shapes of a model of
``--mil_heads L``.  The model is ``mil.MILClassifier(..., levels=(1, 2, 3))``; it carries the registered buffer
``aggregator.levels`` (int64[L], the pyramid levels), and a state_dict is a levels model if it holds that key.  Every row has a
level SLOT ``level_of[i]`` in 0..L-1 (the position of its pyramid level in ``aggregator.levels``).  This module holds:

* ``levels_forward``: ``hipac_mil_levels_forward`` -- many bags of contiguous rows scored in one call (inference).
* ``load_mil_levels_library``: the bound library; ``mil_train.NativeMILTrainer`` runs ``hipac_mil_levels_train_fwd_bwd``
  through it when its model is a levels model.
* ``host_forward``: the same model in plain torch (masked scores), what ``MILClassifier`` runs on a CPU tensor.
* ``load_triples`` / ``epoch_batches``: one feature matrix over the triples of the chosen levels, bags by slide, and the
  per-(bag, level) sampling of ``--mil_bag_size``.

A model without ``aggregator.levels`` never comes here.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi

MIL_LEVELS_ABI_VERSION = 1  # include/hipac_mil_levels.h HIPAC_MIL_LEVELS_ABI_VERSION this binding was written against
MAX_LEVELS = 4              # HIPAC_MIL_MAX_LEVELS
LEVELS_KEY = "aggregator.levels"

# name -> (restype, argtypes); must list every symbol include/hipac_mil_levels.h declares (tests/test_mil_levels_capi_symbols.py)
MIL_LEVELS_SYMBOLS = {
    "hipac_mil_levels_abi_version": (C.c_int, []),
    "hipac_mil_levels_forward_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_levels_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hipac_mil_levels_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hipac_mil_levels_train_fwd_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
}

_bound = None


def load_mil_levels_library():
    """The library of ``capi.load_library()`` with the multiscale entry points bound; HipacError on a version mismatch."""
    global _bound
    lib = capi.load_library()
    if _bound is not lib:
        _bound = capi.bind_symbols(lib, MIL_LEVELS_SYMBOLS, "hipac_mil_levels_abi_version", MIL_LEVELS_ABI_VERSION,
                                   "MIL levels ABI")
    return lib


def check_levels(levels) -> Tuple[int, ...]:
    """-> the pyramid levels as a tuple of 1..MAX_LEVELS distinct ints out of 0..3 in ascending order; ValueError otherwise."""
    try:
        out = tuple(int(v) for v in levels)
        same = all(not isinstance(v, bool) and int(v) == v for v in levels)
    except (TypeError, ValueError):
        raise ValueError(f"levels must be a sequence of pyramid levels, got {levels!r}") from None
    if not same or not 1 <= len(out) <= MAX_LEVELS or any(not 0 <= v <= 3 for v in out) or \
            any(b <= a for a, b in zip(out[:-1], out[1:])):
        raise ValueError(f"levels must be 1..{MAX_LEVELS} distinct pyramid levels out of 0..3 in ascending order, got {levels!r}")
    return out


def parse_levels_flag(text: str) -> Tuple[int, ...]:
    """``--mil_levels 1,2,3`` -> (1, 2, 3): two to four distinct levels out of 0..3, ascending; ValueError otherwise."""
    try:
        vals = [int(t) for t in str(text).split(",")]
    except ValueError:
        raise ValueError(f"--mil_levels {text}: give pyramid levels separated by commas, such as 1,2,3") from None
    if len(vals) < 2:
        raise ValueError(f"--mil_levels {text}: give at least two levels (one level is --patch_level L without this flag)")
    if any(not 0 <= v <= 3 for v in vals):
        raise ValueError(f"--mil_levels {text}: the levels are 0, 1, 2 and 3")
    if any(b <= a for a, b in zip(vals[:-1], vals[1:])):
        raise ValueError(f"--mil_levels {text}: give two to four distinct levels in ascending order")
    return tuple(vals)


def model_levels(sd: Dict[str, torch.Tensor]) -> Optional[Tuple[int, ...]]:
    """The pyramid levels of a levels model's state_dict (its ``aggregator.levels`` buffer), None for any other model;
    ValueError when the buffer disagrees with the rows of ``aggregator.attn_U.weight``."""
    if LEVELS_KEY not in sd:
        return None
    levels = check_levels([int(v) for v in sd[LEVELS_KEY].detach().cpu().reshape(-1).tolist()])
    w = sd.get("aggregator.attn_U.weight")
    if w is None or int(w.shape[0]) != len(levels):
        raise ValueError(f"{LEVELS_KEY} names {len(levels)} levels, aggregator.attn_U.weight has "
                         f"{'no' if w is None else int(w.shape[0])} rows")
    return levels


def _check_level_of(level_of, n: int) -> torch.Tensor:
    if level_of is None:
        raise ValueError("a levels model needs level_of: the level slot of every row")
    lv = torch.as_tensor(level_of)
    if lv.dim() != 1 or int(lv.numel()) != n or lv.dtype.is_floating_point or lv.dtype == torch.bool:
        raise ValueError(f"level_of must be an integer vector with one entry per row ({n})")
    if lv.dtype != torch.uint8 and n and (int(lv.min()) < 0 or int(lv.max()) > 255):  # a uint8 vector holds nothing else
        raise ValueError("level_of holds a value outside 0..255")
    return lv


def host_forward(model, feats: torch.Tensor, bag_offsets, level_of) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The levels model in plain torch, differentiable, in the dtype of ``feats``: the L-head scores with every row masked to
    minus infinity in the heads of the other levels, one softmax per (bag, level).  A (bag, level) without rows pools to zeros
    (its column is softmaxed unmasked and multiplied by the all-zero mask: no NaN, in the forward or the gradients).
    -> (logits [n_bags, C], attn [n], pooled [n_bags, L F])."""
    agg = model.aggregator
    L, n = int(agg.attn_U.weight.shape[0]), int(feats.shape[0])
    lv = _check_level_of(level_of, n).to(feats.device, torch.int64)
    offs = [int(v) for v in torch.as_tensor(bag_offsets).reshape(-1).tolist()]
    H = torch.tanh(agg.attn_V(feats))
    S = agg.attn_U(H)                                                                       # [n][L]
    mask = lv[:, None] == torch.arange(L, device=feats.device)[None, :]                     # [n][L]; a row of no level: all False
    pooled, attn = [], []
    for a, b in zip(offs[:-1], offs[1:]):
        m, x = mask[a:b], feats[a:b]
        live = m.any(dim=0, keepdim=True)                                                   # [1][L]
        s = torch.where(m | ~live, S[a:b], torch.full_like(S[a:b], float("-inf")))
        w = torch.softmax(s, dim=0) * m.to(feats.dtype)                                     # [N][L], one nonzero per row
        pooled.append(torch.cat([torch.sum(w[:, k:k + 1] * x, dim=0) for k in range(L)]))
        attn.append(w.sum(dim=1))
    pooled = torch.stack(pooled)
    return model.classifier(pooled), torch.cat(attn), pooled


def levels_forward(sd: Dict[str, torch.Tensor], feats: torch.Tensor, bag_offsets, level_of, want_attn: bool = True,
                   want_pooled: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Score many bags at once with a levels model.  ``sd``: MILClassifier state_dict tensors (float32, on the device of
    ``feats``; ``aggregator.levels`` is not needed: L is the rows of ``aggregator.attn_U.weight``); ``feats`` float32[n, F]
    with the rows of a bag contiguous; ``bag_offsets`` int[n_bags + 1] (validated on the host); ``level_of`` int[n], the level
    slot of every row (a value >= L: a row of no level).  -> (logits[n_bags, C], attn[n] or None, pooled[n_bags, L F] or None)."""
    from .mil_heads import mil_heads_params

    capi._require_gpu(feats)
    if feats.dtype != torch.float32 or feats.dim() != 2:
        raise capi.HipacError("feats must be float32[n, feature_dim]")
    n, F = int(feats.shape[0]), int(feats.shape[1])
    offs_host, _ = capi.check_bag_offsets(bag_offsets, n)
    lv = _check_level_of(level_of, n)
    lib = load_mil_levels_library()
    p, L = mil_heads_params(sd, F, feats.device)  # the shapes of a model of L heads
    if L > MAX_LEVELS:
        raise capi.HipacError(f"aggregator.attn_U.weight has {L} rows: 1..{MAX_LEVELS} levels are supported")
    lv_dev = lv.to(feats.device, torch.uint8).contiguous()
    return capi._mil_head_forward(lib, "hipac_mil_levels_forward", "hipac_mil_levels_forward_workspace_bytes", p, L, feats, offs_host,
                                  (lv_dev.data_ptr(),), n if want_attn else None, L * F if want_pooled else 0, "multiscale")


# ----------------------------------------------------------------------------
# bags over several levels
# ----------------------------------------------------------------------------
def triple_names(level: int, data_dir: str = ".") -> Tuple[str, str, str]:
    """The (features, labels, paths) files ``--extract_features --patch_level level`` writes."""
    return tuple(f if data_dir in ("", ".") else os.path.join(data_dir, f) for f in (f"patch_features_{level}.npy", f"patch_labels_{level}.npy",
                                                     f"patch_paths_{level}.txt"))


def load_triples(levels: Sequence[int], data_dir: str = ".", verbose: bool = True):
    """The triples of the chosen pyramid levels as one bag set by slide.
    -> (features float32[N, F]: the matrices concatenated in ascending level order; level_of uint8[N]: the level slot of every
    feature row; order, offsets, slide names, slide labels as ``mil.group_patches_by_wsi(..., by_slide=True)`` gives them over
    the concatenated paths; starts int64[L + 1]: level slot k owns the feature rows starts[k] .. starts[k + 1] - 1, row
    starts[k] + i being line i of its paths file).
    Inside a bag the rows are sorted by level and keep their file order inside a level.  A slide's label is 1 if any of its
    rows at any chosen level is tumour.  A slide that has no patch at some level keeps its other levels; the count of such
    slides is reported once per level.  ValueError when the feature dims of the levels differ or a triple does not agree."""
    from .mil import group_patches_by_wsi

    levels = check_levels(levels)
    mats, labels, paths, starts = [], [], [], [0]
    for level in levels:
        fp, lp, pp = triple_names(level, data_dir)
        f, l = np.load(fp), np.load(lp)
        with open(pp, "r") as fh:
            p = [line.strip() for line in fh if line.strip()]
        if f.ndim != 2 or len(p) != f.shape[0] or l.shape[0] != f.shape[0]:
            raise ValueError(f"triple of level {level} does not agree: features {f.shape}, labels {l.shape}, {len(p)} paths")
        if mats and f.shape[1] != mats[0].shape[1]:
            raise ValueError(f"feature dims differ: level {levels[0]} has {mats[0].shape[1]} columns, level {level} has {f.shape[1]}")
        mats.append(np.asarray(f, np.float32)), labels.append(np.asarray(l).astype(np.int64).ravel()), paths.extend(p)
        starts.append(starts[-1] + f.shape[0])
    feats = np.ascontiguousarray(np.concatenate(mats, axis=0), dtype=np.float32)
    starts = np.asarray(starts, np.int64)
    level_of = np.repeat(np.arange(len(levels), dtype=np.uint8), np.diff(starts))
    order, offsets, names, wsi = group_patches_by_wsi(paths, np.concatenate(labels), by_slide=True)
    if verbose:
        bag_of_row = np.repeat(np.arange(len(names)), np.diff(offsets))
        for k, level in enumerate(levels):
            have = np.unique(bag_of_row[level_of[order] == k]).size
            if have < len(names):
                print(f"[INFO] MIL levels: {len(names) - have} of {len(names)} slides have no patch at level {level}; "
                      "they keep their other levels")
    return feats, level_of, order, offsets, names, wsi, starts


def epoch_batches(train_bags: Sequence[int], order: np.ndarray, offsets: np.ndarray, level_of: np.ndarray, n_levels: int, epoch: int,
                  seed: int = 0, bags_per_step: int = 32, bag_size: Optional[int] = None):
    """``mil_train.epoch_batches`` for bags over several levels: a seeded shuffle of the training bags, cut into groups of
    ``bags_per_step``; with ``bag_size`` a seeded sample without replacement of at most that many rows per (bag, LEVEL) -- level
    0 has 64 times the rows of level 3 and would crowd it out of a per-bag sample -- the rows kept in their own order.
    ``level_of``: the level slot of every FEATURE row.  Yields (rows int32[n] into the feature matrix, offsets int64[k + 1],
    bag indices int64[k], level slot uint8[n] of every batch row).  A function of (seed, epoch) only."""
    rng = np.random.default_rng([seed, epoch + 1])
    bags = np.asarray(train_bags, np.int64)[rng.permutation(len(train_bags))]
    for s in range(0, len(bags), bags_per_step):
        group = bags[s:s + bags_per_step]
        rows, offs = [], [0]
        for b in group:
            r = order[offsets[b]:offsets[b + 1]]
            if bag_size is not None:
                lv, keep = level_of[r], np.ones(len(r), bool)
                for k in range(n_levels):
                    at = np.flatnonzero(lv == k)
                    if len(at) > bag_size:
                        keep[at] = False
                        keep[at[rng.choice(len(at), size=bag_size, replace=False)]] = True
                r = r[keep]
            rows.append(r)
            offs.append(offs[-1] + len(r))
        rows = np.concatenate(rows)
        yield rows.astype(np.int32), np.asarray(offs, np.int64), group, np.ascontiguousarray(level_of[rows], dtype=np.uint8)


def attention_tables(attn: np.ndarray, order: np.ndarray, starts: np.ndarray) -> List[np.ndarray]:
    """The attention of the gathered rows (``attn[i]`` belongs to feature row ``order[i]``) as one float32 [patches_L, 1]
    table per level slot, row i belonging to line i of that level's paths file."""
    table = np.zeros(int(starts[-1]), np.float32)
    table[order] = np.asarray(attn, np.float32).reshape(-1)
    return [table[starts[k]:starts[k + 1]].reshape(-1, 1).copy() for k in range(len(starts) - 1)]
