"""A float32 stand-in of the single-head MIL training step (csrc/mil_train.hip, hipac_mil_train_fwd_bwd) and of the
inference head (csrc/mil.hip, hipac_mil_forward) in plain torch ops on the CPU, for tests/test_oracle_mil_edge.py.

Written from the formulas in the two files' header comments, with a MANUAL backward (no autograd):

    H = tanh(X V^T + b_V),  s = H U + b_U,  a = softmax of s inside each bag,  pooled_b = sum a_i x_i  (or mean / max)
    hid = relu(pooled W1^T + b1),  logits = hid W2^T + b2,  loss = sum w[y_b] nll_b / sum w[y_b]
    g_b = dL/dpooled_b,  ds_i = a_i (x_i . g_b - pooled_b . g_b),  dH_i = ds_i U (1 - H_i^2),
    dV = dH^T X,  db_V = sum dH_i,  dU = sum ds_i H_i,  db_U = sum ds_i

It never calls the native code.  Two ends: without a fault it has to pass every gate of tests/mil_edge_cases.py (the gates
are not so tight that only torch's own autograd passes them), and with ``fault=`` it applies exactly ONE of FAULTS, the
mistakes a change to the kernels could make, to show that the cases and metrics notice each.  In float64 the formulas
land on torch's float64 autograd (the test holds them to it), so what separates the float32 stand-in from the reference
is float32 alone.
"""
from __future__ import annotations

import numpy as np
import torch

FAULTS = ("last_attn_unit", "feature_tail", "tile_last_row", "bag_edge", "mean_by_segment", "max_from_zero", "no_max_shift",
          "accumulate_overwrites", "score_group_clamp")
TILE = 64    # rows per tile of the training step
GROUP = 16   # rows per workgroup of the inference score kernel
VW, VB, UW, UB = ("aggregator.attn_V.weight", "aggregator.attn_V.bias", "aggregator.attn_U.weight", "aggregator.attn_U.bias")
W1, B1, W2, B2 = ("classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias")


class StandIn:
    def __init__(self, fault=None, dtype=torch.float32):
        assert fault is None or fault in FAULTS, fault
        self.fault, self.dtype = fault, dtype

    def _forward(self, sd, pooling, x, offsets, inference):
        """x [n][F]: the batch rows in order.  -> everything the backward needs."""
        f = self.fault
        p = {k: v.detach().to(self.dtype) for k, v in sd.items()}
        offs = np.asarray(offsets, dtype=np.int64)
        B, n, F = offs.size - 1, int(offs[-1]), x.shape[1]
        sizes = torch.from_numpy(np.diff(offs))
        # entries: (row, bag) pairs that a bag's softmax and pooling run over -- the batch rows themselves, in order, and
        # under bag_edge the first row of the next bag once more
        ent_row, ent_bag = torch.arange(n), torch.repeat_interleave(torch.arange(B), sizes)
        if f == "bag_edge" and B > 1:
            ent_row = torch.cat([ent_row, torch.from_numpy(offs[1:-1])])
            ent_bag = torch.cat([ent_bag, torch.arange(B - 1)])
        keep = (ent_row % TILE != TILE - 1) if f == "tile_last_row" else torch.ones_like(ent_row, dtype=torch.bool)
        xe = x[ent_row]
        out = {"p": p, "B": B, "n": n, "F": F, "ent_row": ent_row, "ent_bag": ent_bag, "xe": xe, "a": None}
        if pooling == "attention":
            A = p[VW].shape[0]
            live = A - 1 if f == "last_attn_unit" else A
            H = torch.tanh(x @ p[VW][:live].T + p[VB][:live])
            s = H @ p[UW][0, :live] + p[UB][0]
            if inference and f == "score_group_clamp" and n % GROUP:
                s[GROUP * (n // GROUP):] = s[n - 1]
            se = s[ent_row]
            if f == "no_max_shift":
                e = torch.exp(se)
            else:
                mx = torch.full((B,), float("-inf"), dtype=self.dtype).scatter_reduce(0, ent_bag, se, "amax")
                e = torch.exp(se - mx[ent_bag])
            z = torch.zeros(B, dtype=self.dtype).index_add_(0, ent_bag, e)
            a = e / z[ent_bag]
            pooled = torch.zeros(B, F, dtype=self.dtype).index_add_(0, ent_bag[keep], a[keep, None] * xe[keep])
            out.update(H=H, live=live, a=a)
        elif pooling == "mean":
            cnt = sizes.clone()
            if f == "mean_by_segment":  # the rows of the bag's last segment
                cnt = torch.from_numpy(offs[1:] - np.maximum(offs[:-1], TILE * ((offs[1:] - 1) // TILE)))
            pooled = torch.zeros(B, F, dtype=self.dtype).index_add_(0, ent_bag[keep], xe[keep]) / cnt.to(self.dtype)[:, None]
        else:
            init = 0.0 if f == "max_from_zero" else float("-inf")
            pooled = torch.full((B, F), init, dtype=self.dtype).scatter_reduce(0, ent_bag[keep, None].expand(-1, F), xe[keep], "amax")
        hid = torch.relu(pooled @ p[W1].T + p[B1])
        out.update(pooled=pooled, hid=hid, logits=hid @ p[W2].T + p[B2])
        return out

    def infer(self, sd, pooling, x, offsets):
        """hipac_mil_forward: -> (logits [B][C], attn [n] or None, pooled [B][F])."""
        o = self._forward(sd, pooling, x.to(self.dtype), offsets, True)
        return o["logits"], (None if o["a"] is None else o["a"][:o["n"]]), o["pooled"]

    def step(self, sd, pooling, feats, rows, offsets, labels, cw, prev=None):
        """hipac_mil_train_fwd_bwd: -> (loss, logits, gradients by state_dict key, attn [n] or None).  ``prev``: the gradient
        buffers' contents before an accumulating call."""
        f = self.fault
        x = feats.to(self.dtype)
        if rows is not None:
            x = x[rows.long()]
        o = self._forward(sd, pooling, x, offsets, False)
        p, B, n, F, ent_bag, xe = o["p"], o["B"], o["n"], o["F"], o["ent_bag"], o["xe"]
        logits, hid, pooled = o["logits"], o["hid"], o["pooled"]
        y, r = labels.long(), torch.arange(B)
        mx = logits.max(dim=1).values
        e = torch.exp(logits - mx[:, None])
        se = e.sum(dim=1)
        nll = torch.log(se) + mx - logits[r, y]
        wy = torch.ones(B, dtype=self.dtype) if cw is None else cw.to(self.dtype)[y]
        den = wy.sum()
        loss = (wy * nll).sum() / den
        dl = e / se[:, None]
        dl[r, y] -= 1.0
        dl = dl * (wy / den)[:, None]
        grads = {W2: dl.T @ hid, B2: dl.sum(dim=0)}
        dhid = (dl @ p[W2]) * (hid > 0)
        grads[W1], grads[B1] = dhid.T @ pooled, dhid.sum(dim=0)
        attn = None
        if pooling == "attention":
            a, H, live = o["a"], o["H"][o["ent_row"]], o["live"]
            g = dhid @ p[W1]
            xg = (xe * g[ent_bag]).sum(dim=1)
            cdot = torch.zeros(B, dtype=self.dtype).index_add_(0, ent_bag, a * xg)  # pooled_b . g_b = sum_j a_j (x_j . g_b)
            ds = a * (xg - cdot[ent_bag])
            dH = ds[:, None] * p[UW][0, :live] * (1.0 - H * H)
            A = p[VW].shape[0]
            dV, dbV, dU = (torch.zeros(A, F, dtype=self.dtype), torch.zeros(A, dtype=self.dtype), torch.zeros(1, A, dtype=self.dtype))
            dV[:live], dbV[:live], dU[0, :live] = dH.T @ xe, dH.sum(dim=0), (ds[:, None] * H).sum(dim=0)
            if f == "feature_tail":
                dV[:, TILE * (F // TILE):] = 0.0
            grads.update({VW: dV, VB: dbV, UW: dU, UB: ds.sum().reshape(1)})
            attn = a[:n]
        if prev is not None:
            for k in grads:
                if not (f == "accumulate_overwrites" and k == VB):
                    grads[k] = prev[k].to(self.dtype) + grads[k]
        return loss, logits, grads, attn
