"""Inputs and the torch yardstick shared by tests/test_mil_gated_host.py, tests/test_gpu_mil_gated.py and
tests/tools/measure_mil_gated_fp32.py.

The yardstick is ``Twin`` below: gated attention pooling (Ilse et al. 2018, eq. 9) with K heads written in plain torch --
three nn.Linears in the aggregator, the forward lines, and the classifier.  It does not import ``mil.MILAttentionPooling``;
the module under test is checked against it, in float64 for the GPU tests and in float32 for the measurement that sets
their gates."""
import copy

import numpy as np
import torch
import torch.nn as nn

# the bag sizes of mil_heads_cases.SIZES: bags of one row, bags either side of the 64-row tile and of the softmax's
# 256-thread stride, tiles that hold several bags, one bag spanning 65 tiles; n = 5714
SIZES = [1, 2, 63, 64, 65, 129, 257, 1000, 4133]
# (F, A, hidden, C, K): the reference dims with one head and with the yaml's head count; A no multiple of 32 (A_pad = 96:
# the pad columns of both planes), odd K and three classes; A and hidden at their limits; A_pad = 64 and A_pad = 160, the
# one-tile and the three-tile variant of the weight-gradient kernel (the others take the two-tile one, in one workgroup column
# or in two), the first with F no multiple of the 32-column K step or the 64-column block
DIMS = [(512, 128, 128, 2, 1), (512, 128, 128, 2, 8), (128, 72, 32, 3, 3), (1024, 256, 256, 2, 2), (72, 40, 16, 2, 2),
        (192, 160, 48, 2, 3)]
ACC_SIZES = [300, 40, 7, 2048]  # mil_heads_cases.ACC_SIZES: the second batch of the accumulate test
ACC_DIMS = DIMS[1]


class TwinPooling(nn.Module):
    def __init__(self, F, A, K):
        super().__init__()
        self.heads = K
        self.attn_V = nn.Linear(F, A)
        self.attn_U = nn.Linear(A, K)
        self.attn_G = nn.Linear(F, A)

    def forward(self, x):
        Hg = torch.tanh(self.attn_V(x)) * torch.sigmoid(self.attn_G(x))                          # [N][A]
        S = self.attn_U(Hg)                                                                      # [N][K]
        a = torch.softmax(S, dim=0)                                                              # per head, over the bag
        M = torch.stack([torch.sum(a[:, k:k + 1] * x, dim=0) for k in range(self.heads)])        # M[k] = sum_i a[i][k] x[i]
        return M.reshape(-1), a                                                                  # head-major


class Twin(nn.Module):
    """Same parameter names, shapes and construction order as ``mil.MILClassifier(..., heads=K, gated=True)``."""

    def __init__(self, F, A, hidden, C, K):
        super().__init__()
        self.aggregator = TwinPooling(F, A, K)
        self.classifier = nn.Sequential(nn.Linear(K * F, hidden), nn.ReLU(), nn.Linear(hidden, C))

    def forward(self, x):
        pooled, a = self.aggregator(x)
        return self.classifier(pooled), a


def case_list():
    """(id, dims, weighted, permuted): the reference dims (K = 1 and K = 8) under {class weights} x {row index}; the other
    dims weighted and permuted."""
    out = [(f"K{d[4]}-{'w' if w else 'nw'}-{'perm' if p else 'id'}", d, w, p) for d in DIMS[:2] for w in (False, True)
           for p in (False, True)]
    for dims in DIMS[2:]:
        out.append((f"K{dims[4]}-F{dims[0]}", dims, True, True))
    return out


def group_key(dims):
    return ",".join(map(str, dims))


def make_twin(dims, seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    return Twin(*dims).to(dtype).train()


def retyped(model, dtype):
    m = copy.deepcopy(model).to(dtype)
    m.zero_grad()
    return m


def make_inputs(dims, permuted, sizes=SIZES, seed=0):
    """mil_heads_cases.make_inputs' recipe: feats float32[N, F] (0.7 randn), rows int32[n] (a permuted, sub-sampled index)
    or None, offsets int64[B + 1], labels int64[B], class weights [C]."""
    F, C = dims[0], dims[3]
    g = torch.Generator().manual_seed(1000 + seed)
    n = int(sum(sizes))
    N = n + 1234 if permuted else n
    feats = 0.7 * torch.randn(N, F, generator=g)
    rows = torch.randperm(N, generator=g)[:n].to(torch.int32) if permuted else None
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    labels = torch.tensor([(i * 7 + i // 3) % C for i in range(len(sizes))], dtype=torch.int64)
    cw = torch.tensor([1.0, 2.5, 0.6, 1.7][:C])
    return feats, rows, offsets, labels, cw


def accumulate_inputs(dims):
    return make_inputs(dims, True, seed=1), make_inputs(dims, False, sizes=ACC_SIZES, seed=2)


def reference(twin_f32, feats, rows, offsets, labels, cw, dtype):
    """One training step of the twin in ``dtype`` on the CPU -> (loss, logits [B, C], attention [n, K], gradients)."""
    m = retyped(twin_f32, dtype).train()
    x = feats.to(dtype)
    if rows is not None:
        x = x[rows.long()]
    outs = [m(x[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    logits = torch.stack([o[0] for o in outs])
    loss = nn.CrossEntropyLoss(weight=None if cw is None else cw.to(dtype))(logits, labels)
    loss.backward()
    attn = torch.cat([o[1] for o in outs]).detach()
    return loss.detach(), logits.detach(), attn, {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def eval_reference(twin_f32, feats, offsets, dtype):
    """The twin's forward without gradients -> (logits [B, C], attention [n, K], pooled [B, K F])."""
    m = retyped(twin_f32, dtype).eval()
    x = feats.to(dtype)
    with torch.no_grad():
        pooled, attn = zip(*[m.aggregator(x[a:b]) for a, b in zip(offsets[:-1], offsets[1:])])
        pooled = torch.stack(pooled)
        return m.classifier(pooled), torch.cat(attn), pooled


def rel(a, b):
    """max|a - b| / max|b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())
