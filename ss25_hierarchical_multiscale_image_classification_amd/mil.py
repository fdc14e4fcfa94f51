"""Host-side mirror of the reference's MIL pieces.

* ``MILAttentionPooling`` / ``MILClassifier`` -- src/models/mil_classifier.py:5-45: same
  constructor arguments, ``forward(bag) -> (logits, attention)`` shapes and state_dict keys
  (``aggregator.attn_V.*``, ``aggregator.attn_U.*``, ``classifier.0.*``, ``classifier.2.*``).
  In ``eval()`` mode ``forward`` runs ``hipac_mil_forward`` (HIP) -- a CPU tensor raises, there is
  no CPU fallback; in ``train()`` mode it runs the ordinary autograd graph, under the dropout masks of
  ``mil_dropout.host_mask`` when ``dropout > 0`` (applied functionally: no module, no new state_dict key).
  ``forward_bags`` scores MANY bags in one launch pair (the reference loops over bags).
  ``heads=K`` (1..8, the yaml's ``attention_heads``) is multi-head attention pooling: ``attn_U`` is ``Linear(attn_dim, K)``,
  one softmax per head, the K pooled vectors concatenated in front of ``classifier.0`` = ``Linear(K * feature_dim, hidden)``;
  same keys, and ``eval()`` runs ``hipac_mil_heads_forward`` (``mil_heads.py``) when K > 1.  K = 1 is the reference's model.
  ``gated=True`` is the gated attention of Ilse et al. 2018 (eq. 9, the form CLAM uses): the aggregator gains
  ``attn_G = Linear(in_dim, attn_dim)`` (keys ``aggregator.attn_G.weight`` / ``.bias``, constructed last, so an ungated model
  draws the same numbers and has the same keys as before) and scores a patch with ``attn_U(tanh(attn_V(x)) * sigmoid(attn_G(x)))``;
  ``eval()`` runs ``hipac_mil_gated_forward`` (``mil_gated.py``) for any K.  A saved model is gated if it has the keys.
  ``levels=(1, 2, 3)`` is the multiscale model of ``mil_levels.py``: a bag holds rows of L pyramid levels, ``attn_U`` has one
  branch per level and every level its own softmax over its rows of the bag; the shapes are those of ``heads=L``, plus the
  registered buffer ``aggregator.levels`` (int64[L]) by which a saved model is recognised.  ``forward`` / ``forward_bags`` then
  take ``level_of`` (the level slot of every row); a GPU tensor runs ``hipac_mil_levels_forward``, a CPU tensor plain torch.
* ``group_patches_by_wsi`` / ``WSIMILDDataset`` -- src/datasets/mildataset.py:6-47.  By default the
  bag key is the reference's as written: ``'_'.join(basename.split('_')[:-2])``, which for the patch
  names ``{slide}_x{x}_y{y}_{label}.png`` keeps the ``_x{x}`` field (one bag per slide COLUMN);
  ``by_slide=True`` drops it, which is what the reference's comment describes.
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import capi


def group_patches_by_wsi(paths: Sequence[str], labels: Sequence[int], by_slide: bool = False
                         ) -> Tuple[np.ndarray, np.ndarray, List[str], np.ndarray]:
    """-> (order int64[n]: row indices sorted by bag, first-appearance bag order, original row order
    inside a bag; offsets int64[n_bags+1]; bag names; wsi_labels int64[n_bags] = any member label == 1)."""
    drop = 3 if by_slide else 2
    index, rows, wsi = {}, [], []
    for i, p in enumerate(paths):
        key = "_".join(os.path.basename(p).split("_")[:-drop])
        b = index.setdefault(key, len(index))
        if b == len(rows):
            rows.append([]), wsi.append(0)
        rows[b].append(i)
        if int(labels[i]) == 1:
            wsi[b] = 1
    order = np.array([i for r in rows for i in r], np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return order, offsets, list(index.keys()), np.array(wsi, np.int64)


class WSIMILDDataset(torch.utils.data.Dataset):
    """src/datasets/mildataset.py:6-47: bags from the (features .npy, labels .npy, paths .txt) triple that
    ``--extract_features`` writes.  ``__getitem__ -> (features float32[n_i,F], wsi_label int64 scalar)``.
    The files are this repository's own output or the user's: ``allow_pickle`` stays off."""

    def __init__(self, features_path, labels_path, paths_path, by_slide: bool = False):
        self.features = np.load(features_path)
        self.labels = np.load(labels_path)
        with open(paths_path, "r") as f:
            self.paths = [line.strip() for line in f]
        self.order, self.offsets, self.names, wsi = group_patches_by_wsi(self.paths, self.labels, by_slide)
        self.wsi_data = [{"features": torch.tensor(self.features[self.order[a:b]], dtype=torch.float32),
                          "patch_labels": torch.tensor(self.labels[self.order[a:b]], dtype=torch.long),
                          "wsi_label": torch.tensor(int(w), dtype=torch.long)}
                         for a, b, w in zip(self.offsets[:-1], self.offsets[1:], wsi)]

    def __len__(self):
        return len(self.wsi_data)

    def __getitem__(self, idx):
        return self.wsi_data[idx]["features"], self.wsi_data[idx]["wsi_label"]


class MILAttentionPooling(nn.Module):
    """mil_classifier.py:5-18 (ABMIL, Ilse et al.).  ``heads`` = K attention branches over the shared hidden layer
    (the yaml's ``attention_heads``): ``attn_U`` is ``Linear(attn_dim, K)``, the softmax runs per head over the bag, and
    ``forward`` returns the K pooled vectors concatenated head-major (K * in_dim) and the attention (N, K).  K = 1 is
    the reference's module.  ``gated``: the score is ``attn_U(tanh(attn_V(x)) * sigmoid(attn_G(x)))`` (Ilse et al. eq. 9);
    ``attn_G`` is constructed after the other two, and only then.  ``levels`` (pyramid levels, ascending): one branch per
    level (``heads`` = their number) and the buffer ``levels``; ``forward`` then needs ``level_of``."""

    def __init__(self, in_dim, attn_dim=128, heads=1, gated=False, levels=None):
        super().__init__()
        from .mil_heads import check_heads

        self.heads, self.gated = check_heads(heads), bool(gated)
        self.attn_V = nn.Linear(in_dim, attn_dim)
        self.attn_U = nn.Linear(attn_dim, self.heads)
        if self.gated:
            self.attn_G = nn.Linear(in_dim, attn_dim)
        if levels is not None:
            self.register_buffer("levels", torch.tensor(list(levels), dtype=torch.int64))

    def forward(self, x):
        if self.gated:
            a = torch.softmax(self.attn_U(torch.tanh(self.attn_V(x)) * torch.sigmoid(self.attn_G(x))), dim=0)
        else:
            a = torch.softmax(self.attn_U(torch.tanh(self.attn_V(x))), dim=0)
        # M[k] = sum_i a[i][k] x[i]; for one head this is the reference's torch.sum(a * x, dim=0), bit for bit
        pooled = torch.stack([torch.sum(a[:, k:k + 1] * x, dim=0) for k in range(self.heads)])
        return pooled.reshape(-1), a


class MILClassifier(nn.Module):
    """mil_classifier.py:20-45.  ``heads`` > 1 (attention pooling only): multi-head attention pooling, ``classifier.0``
    takes ``heads * feature_dim`` columns; the state_dict keys are the same.  ``attn_dim`` / ``hidden_dim`` are the
    reference's 128 unless given.  ``gated`` (attention pooling only): gated attention, two more keys
    (``aggregator.attn_G.weight`` [attn_dim][feature_dim], ``aggregator.attn_G.bias`` [attn_dim]); refused together with ``dropout`` > 0.
    ``levels`` (attention pooling only; not with ``heads`` > 1, ``gated`` or ``dropout``): the multiscale model of
    ``mil_levels.py`` over these pyramid levels, in the shapes of ``heads = len(levels)`` plus the buffer ``aggregator.levels``."""

    def __init__(self, feature_dim, num_classes=2, pooling="attention", dropout=0.0, dropout_seed=0, heads=1, attn_dim=128,
                 hidden_dim=128, gated=False, levels=None):
        super().__init__()
        from .mil_heads import check_heads

        if pooling not in ("attention", "mean", "max"):
            raise ValueError("Unknown pooling: choose from 'attention', 'mean', 'max'")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("dropout must satisfy 0 <= p < 1")
        self.heads = check_heads(heads)
        if self.heads != 1 and pooling != "attention":
            raise ValueError(f"heads = {self.heads} needs attention pooling: {pooling} pooling has no attention to branch")
        self.gated = bool(gated)
        if self.gated and pooling != "attention":
            raise ValueError(f"gated = True needs attention pooling: {pooling} pooling has no attention to gate")
        if self.gated and float(dropout) > 0.0:
            raise ValueError("gated = True does not go with dropout: the masked step and the Monte-Carlo pass are single-head and ungated")
        self.levels = None
        if levels is not None:
            from .mil_levels import check_levels

            self.levels = check_levels(levels)
            if pooling != "attention":
                raise ValueError(f"levels needs attention pooling: {pooling} pooling has no attention branch per level")
            if self.heads != 1 or self.gated or float(dropout) > 0.0:
                raise ValueError("levels does not go with heads > 1, gated = True or dropout: every level has one ungated branch")
            self.heads = len(self.levels)
        self.pooling = pooling
        # plain attributes, not parameters or buffers: the state_dict keeps the reference's keys.  dropout_step is the
        # mask's sample index (the trainer's step number); the caller advances it.
        self.dropout, self.dropout_seed, self.dropout_step = float(dropout), int(dropout_seed), 0
        if pooling == "attention":
            self.aggregator = MILAttentionPooling(feature_dim, attn_dim, self.heads, self.gated, self.levels)
        self.classifier = nn.Sequential(nn.Linear(self.heads * feature_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, num_classes))

    def _aggregate(self, bag):
        if self.pooling == "attention":
            return self.aggregator(bag)
        return (bag.mean(dim=0), None) if self.pooling == "mean" else (bag.max(dim=0)[0], None)

    def forward_bags(self, feats: torch.Tensor, bag_offsets, want_pooled: bool = False, level_of=None):
        """HIP path for many bags: feats float32[n,F] (bag rows contiguous, on a ROCm device),
        bag_offsets int[n_bags+1] -> (logits[n_bags,C], attn[n] or None[, pooled[n_bags,F]]).  A model of K > 1 heads
        (the rows of ``aggregator.attn_U.weight``) runs ``hipac_mil_heads_forward``: attn[n,K], pooled[n_bags,K F].  A gated
        model (one with ``aggregator.attn_G.weight``) runs ``hipac_mil_gated_forward`` for any K: attn[n,K].  A levels model
        (one with ``aggregator.levels``) needs ``level_of`` int[n], the level slot of every row, and gives attn[n],
        pooled[n_bags,L F]: ``hipac_mil_levels_forward`` on a GPU tensor, ``mil_levels.host_forward`` (plain torch, differentiable)
        on a CPU tensor.  Any other model refuses ``level_of``."""
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        offs = torch.as_tensor(np.asarray(bag_offsets)) if not torch.is_tensor(bag_offsets) else bag_offsets
        if (level_of is not None) != ("aggregator.levels" in sd):
            raise ValueError("level_of goes with a levels model (one with aggregator.levels), and such a model needs it")
        if level_of is not None:
            from .mil_levels import host_forward, levels_forward

            if torch.is_tensor(feats) and not feats.is_cuda:
                logits, attn, pooled = host_forward(self, feats, offs, level_of)
            else:
                logits, attn, pooled = levels_forward(sd, feats.contiguous(), offs, level_of, want_pooled=want_pooled)
        elif self.pooling == "attention" and "aggregator.attn_G.weight" in sd:
            from .mil_gated import gated_forward

            logits, attn, pooled = gated_forward(sd, feats.contiguous(), offs, want_pooled=want_pooled)
        elif self.pooling == "attention" and int(sd["aggregator.attn_U.weight"].shape[0]) != 1:
            from .mil_heads import heads_forward

            logits, attn, pooled = heads_forward(sd, feats.contiguous(), offs, want_pooled=want_pooled)
        else:
            logits, attn, pooled = capi.mil_forward(sd, self.pooling, feats.contiguous(), offs, want_pooled=want_pooled)
        return (logits, attn, pooled) if want_pooled else (logits, attn)

    def forward(self, bag, row0=0, bag_index=0, level_of=None):
        """bag: (num_patches, feature_dim) -> (logits (num_classes), attention (num_patches, heads) or None).  ``row0`` (the
        position of the bag's first row in the batch) and ``bag_index`` place the bag in the dropout masks; they matter in
        ``train()`` mode with ``dropout > 0`` only.  A levels model needs ``level_of`` (see ``forward_bags``); its attention is
        (num_patches, 1), and in ``train()`` mode it runs ``mil_levels.host_forward``."""
        if self.levels is not None:
            if self.training:
                from .mil_levels import host_forward

                logits, attn, _ = host_forward(self, bag, [0, bag.shape[0]], level_of)
            else:
                logits, attn = self.forward_bags(bag, torch.tensor([0, bag.shape[0]]), level_of=level_of)
            return logits[0], attn.reshape(bag.shape[0], 1)
        if level_of is not None:
            raise ValueError("level_of goes with a levels model (one with aggregator.levels)")
        if self.training:
            if self.dropout > 0.0:
                from .mil_dropout import host_dropout

                p, seed, step = self.dropout, self.dropout_seed, self.dropout_step
                pooled, attn = self._aggregate(host_dropout(bag, p, seed, step, 0, row0))
                hid = host_dropout(self.classifier[1](self.classifier[0](pooled)), p, seed, step, 1, bag_index)
                return self.classifier[2](hid), attn
            pooled, attn = self._aggregate(bag)
            return self.classifier(pooled), attn
        logits, attn = self.forward_bags(bag, torch.tensor([0, bag.shape[0]]))
        return logits[0], (None if attn is None else attn.reshape(bag.shape[0], -1))

    def predict(self, bag):
        """Class probabilities of one bag (the reference's ``predict`` does not run as written: it applies a
        numpy softmax to the (logits, attn) tuple, mil_classifier.py:47-50; this is its evident intent)."""
        logits, _ = self.forward(bag)
        return torch.softmax(logits.float(), dim=-1)
