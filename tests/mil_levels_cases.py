"""Inputs and the torch yardstick shared by tests/test_mil_levels_host.py, tests/test_gpu_mil_levels.py and
tests/tools/measure_mil_levels_fp32.py.

The yardstick is ``Twin`` below: the model of ``mil.MILClassifier(heads=L)`` -- two nn.Linears in the aggregator, the L-head
scores, one softmax per head over the bag, the classifier over the L pooled vectors -- with row i's scores set to minus
infinity in the heads other than ``lev(i)``, written in plain torch.  A head whose every score is minus infinity (the bag has
no row of that level) is not softmaxed: its pooled vector is zero.  It does not import ``mil`` or ``mil_levels``; the module
under test is checked against it, in float64 for the GPU tests and in float32 for the measurement that sets their gates."""
import copy

import numpy as np
import torch
import torch.nn as nn

# one batch of five bags, 323 rows, six 64-row tiles: a bag of one row, bag boundaries before (63), on (128) and after (193)
# a tile edge, and a bag spanning three tiles
SIZES = [1, 63, 64, 65, 130]
# (F, A, hidden, C, L): the reference dims with all four levels; A no multiple of 32 with three levels and three classes;
# small dims with two levels; A and hidden at their limits
DIMS = [(512, 128, 128, 2, 4), (128, 72, 32, 3, 3), (72, 40, 16, 2, 2), (1024, 256, 256, 2, 2)]
ACC_SIZES = [40, 7, 90]  # the second batch of the accumulate test: rows at seeded random levels
ACC_DIMS = DIMS[0]
EMPTY_BAG = 1            # the bag of 63 rows has no row of the last level
NOISE_ROW = 250          # a row inside the last bag, for the "row of no level" tests


def pyramid_levels(L):
    """The last L of the pyramid levels 0..3: what ``aggregator.levels`` holds for a model of L levels in these tests."""
    return tuple(range(4 - L, 4))


def level_slots(L, sizes=SIZES, seed=None):
    """The level slot of every batch row, uint8[n].  With ``seed``: random.  Else, for the five bags of SIZES:
    bag 0 (1 row): level 0; bag 1 (63): sorted by level over the levels 0 .. L - 2, none of level L - 1 (for L = 2 that is one
    level); bag 2 (64): every row at level L - 1; bag 3 (65): interleaved row by row, i mod L; bag 4 (130): sorted by level,
    in unequal shares."""
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        return torch.randint(0, L, (int(sum(sizes)),), generator=g).to(torch.uint8)
    assert list(sizes) == SIZES
    out = [np.zeros(1, np.uint8)]
    out.append(np.sort(np.arange(63) % max(L - 1, 1)).astype(np.uint8))
    out.append(np.full(64, L - 1, np.uint8))
    out.append((np.arange(65) % L).astype(np.uint8))
    cuts = np.linspace(0, 1, L + 1) ** 2 * 130  # 0, 8, 32, 73, 130 for L = 4
    out.append(np.repeat(np.arange(L, dtype=np.uint8), np.diff(np.round(cuts).astype(int))))
    lv = np.concatenate(out)
    assert lv.shape == (323,)
    return torch.from_numpy(lv)


class TwinPooling(nn.Module):
    def __init__(self, F, A, L):
        super().__init__()
        self.heads = L
        self.attn_V = nn.Linear(F, A)
        self.attn_U = nn.Linear(A, L)

    def forward(self, x, lev):
        S = self.attn_U(torch.tanh(self.attn_V(x)))                                              # [N][L]
        other = lev.long()[:, None] != torch.arange(self.heads)[None, :]                         # the heads of the other levels
        S = S.masked_fill(other, float("-inf"))
        M, attn = [], torch.zeros(x.shape[0], dtype=x.dtype)
        for k in range(self.heads):
            if bool(other[:, k].all()):                                                          # no row of this level
                M.append(torch.zeros(x.shape[1], dtype=x.dtype))
                continue
            a = torch.softmax(S[:, k], dim=0)                                                    # exactly 0 on the masked rows
            M.append(torch.sum(a[:, None] * x, dim=0))
            attn = attn + a
        return torch.cat(M), attn                                                                # level-major


class Twin(nn.Module):
    """Same parameter names, shapes and construction order as ``mil.MILClassifier(..., heads=L)``."""

    def __init__(self, F, A, hidden, C, L):
        super().__init__()
        self.aggregator = TwinPooling(F, A, L)
        self.classifier = nn.Sequential(nn.Linear(L * F, hidden), nn.ReLU(), nn.Linear(hidden, C))

    def forward(self, x, lev):
        pooled, a = self.aggregator(x, lev)
        return self.classifier(pooled), a


def case_list():
    """(id, dims, weighted, permuted): the reference dims under {class weights} x {row index}; the other dims weighted and
    permuted."""
    out = [(f"L{DIMS[0][4]}-{'w' if w else 'nw'}-{'perm' if p else 'id'}", DIMS[0], w, p) for w in (False, True) for p in (False, True)]
    for dims in DIMS[1:]:
        out.append((f"L{dims[4]}-F{dims[0]}", dims, True, True))
    return out


def group_key(dims):
    return ",".join(map(str, dims))


def make_twin(dims, seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    return Twin(*dims).to(dtype).train()


def levels_state_dict(twin):
    """The twin's parameters as the state_dict of a levels model: plus the ``aggregator.levels`` buffer."""
    sd = {k: v.detach().clone() for k, v in twin.state_dict().items()}
    sd["aggregator.levels"] = torch.tensor(pyramid_levels(twin.aggregator.heads), dtype=torch.int64)
    return sd


def retyped(model, dtype):
    m = copy.deepcopy(model).to(dtype)
    m.zero_grad()
    return m


def make_inputs(dims, permuted, sizes=SIZES, seed=0, level_seed=None):
    """mil_heads_cases.make_inputs' recipe plus the level slots: feats float32[N, F] (0.7 randn), rows int32[n] (a permuted,
    sub-sampled index) or None, offsets int64[B + 1], labels int64[B], class weights [C], level_of uint8[n] (by batch row)."""
    F, C, L = dims[0], dims[3], dims[4]
    g = torch.Generator().manual_seed(1000 + seed)
    n = int(sum(sizes))
    N = n + 77 if permuted else n
    feats = 0.7 * torch.randn(N, F, generator=g)
    rows = torch.randperm(N, generator=g)[:n].to(torch.int32) if permuted else None
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    labels = torch.tensor([(i * 7 + i // 3) % C for i in range(len(sizes))], dtype=torch.int64)
    cw = torch.tensor([1.0, 2.5, 0.6, 1.7][:C])
    return feats, rows, offsets, labels, cw, level_slots(L, sizes, level_seed)


def accumulate_inputs(dims):
    return make_inputs(dims, True, seed=1), make_inputs(dims, False, sizes=ACC_SIZES, seed=2, level_seed=5)


def reference(twin_f32, feats, rows, offsets, labels, cw, level_of, dtype):
    """One training step of the twin in ``dtype`` on the CPU -> (loss, logits [B, C], attention [n], gradients)."""
    m = retyped(twin_f32, dtype).train()
    x = feats.to(dtype)
    if rows is not None:
        x = x[rows.long()]
    outs = [m(x[a:b], level_of[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    logits = torch.stack([o[0] for o in outs])
    loss = nn.CrossEntropyLoss(weight=None if cw is None else cw.to(dtype))(logits, labels)
    loss.backward()
    attn = torch.cat([o[1] for o in outs]).detach()
    return loss.detach(), logits.detach(), attn, {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def eval_reference(twin_f32, feats, offsets, level_of, dtype):
    """The twin's forward without gradients -> (logits [B, C], attention [n], pooled [B, L F])."""
    m = retyped(twin_f32, dtype).eval()
    x = feats.to(dtype)
    with torch.no_grad():
        pooled, attn = zip(*[m.aggregator(x[a:b], level_of[a:b]) for a, b in zip(offsets[:-1], offsets[1:])])
        pooled = torch.stack(pooled)
        return m.classifier(pooled), torch.cat(attn), pooled


def rel(a, b):
    """max|a - b| / max|b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())
