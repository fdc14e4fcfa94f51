"""Developer tool (GPU box): what the k-NN probe of --validate --validate_knn (knn.py, csrc/knn.hip) costs on N x 512 synthetic
feature rows split 80/20, K = 20, beside two yardsticks:
  * what a user without it would run on the same device: normalise, then `torch.mm` over query chunks plus `torch.topk`, the
    chunk sized to 1 GiB of similarities;
  * the float64 restatement on 16 host threads (torch float64 matmul + topk) over a subsample of the queries, scaled to all.
It prints the time of the whole probe (both inverse norms, the search, the vote) and of the search alone, the search's executed
FLOP/s (2 n_q n_b F, padding not counted) as a share of the exact-f32 MFMA peak (157.3 TFLOP/s), the share of queries whose
neighbour lists equal the yardstick's position for position, and the same for a second shape with few queries (1 000 x n_b),
where the bank is cut into column groups.  Medians of `reps` runs after a warm-up, the device synchronised on both sides of
every timed region, the modes alternated run by run.  Not a gate.
usage: python tools/knnbench.py [N] [reps] [--host_queries Q] [--host_reps R] [--no_host]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ss25_hierarchical_multiscale_image_classification_amd import knn, validate  # noqa: E402


def flag(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and not sys.argv[i - 1].startswith("--")]
N = int(pos[0]) if len(pos) > 0 else 1_000_000
reps = int(pos[1]) if len(pos) > 1 else 7
host_queries, host_reps, no_host = flag("--host_queries", 256), flag("--host_reps", 3), "--no_host" in sys.argv
F, K, T, MFMA_F32_PEAK, FEW = 512, 20, 0.07, 157.3e12, 1000
torch.set_num_threads(16)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def alternate(fns, counts):
    """({name: median ms}, {name: last result}) of the callables, run in turn after one warm-up of the device ones."""
    ts, last = {k: [] for k in fns}, {}
    for k, fn in fns.items():
        if k.startswith("device"):
            timed(fn)
    for i in range(max(counts.values())):
        for k, fn in fns.items():
            if i < counts[k]:
                ms, last[k] = timed(fn)
                ts[k].append(ms)
    return {k: median(v) for k, v in ts.items() if v}, last


# two overlapping clusters on top of 24 shared directions of larger variance, drawn on the device
g = torch.Generator(device="cuda").manual_seed(1)
y_dev = (torch.rand(N, device="cuda", generator=g) < 0.4).long()
q, _ = torch.linalg.qr(torch.randn(F, 25, device="cuda", generator=g))
X = 0.5 * torch.randn(N, F, device="cuda", generator=g)
X += 2.0 * (y_dev.float() - 0.5)[:, None] * q[:, 0]
X += (1.5 * torch.randn(N, 24, device="cuda", generator=g)) @ q[:, 1:].T
y = y_dev.cpu().numpy()
train, test = validate.stratified_split(y, 42)
cw = validate.balanced_class_weights(y[train])
train_dev = torch.from_numpy(train.astype(np.int32)).to("cuda")
test_dev = torch.from_numpy(test.astype(np.int32)).to("cuda")
print(f"== {N} x {F} float32, {train.size} bank rows, {test.size} queries, K = {K}, {reps} runs")


def device_probe(q_rows):
    return knn.knn_classify(X, y_dev, train_dev, q_rows, K, T, cw)


def device_search(q_rows, qs, bs):
    return knn.topk(X, K, q_rows=q_rows, b_rows=train_dev, q_scale=qs, b_scale=bs, check_rows=False)


def torch_probe(q_rows):
    """normalise, chunked mm + topk (1 GiB of similarities per chunk), the same vote in torch"""
    bank = torch.nn.functional.normalize(X[train_dev.long()], dim=1, eps=1e-12)
    qn = torch.nn.functional.normalize(X[q_rows.long()], dim=1, eps=1e-12)
    chunk = max(1, (1 << 30) // (4 * bank.shape[0]))
    sims, idxs = [], []
    for s in range(0, qn.shape[0], chunk):
        v, i = torch.topk(torch.mm(qn[s:s + chunk], bank.T), K, dim=1)
        sims.append(v)
        idxs.append(i)
    sim, idx = torch.cat(sims), torch.cat(idxs)
    w = torch.exp((sim.double() - sim[:, :1].double()) / T)
    lab = y_dev[train_dev.long()][idx]
    s1, s0 = cw[1] * (w * (lab == 1)).sum(1), cw[0] * (w * (lab == 0)).sum(1)
    return {"idx": idx, "pred": (s1 > s0).int()}


def host_probe(q_rows_host):
    """float64 on the host: all bank rows, a subsample of the queries"""
    xb = X[train_dev.long()].cpu().double()
    xq = X[torch.from_numpy(q_rows_host).cuda().long()].cpu().double()
    xb = xb / xb.norm(dim=1, keepdim=True).clamp_min(1e-12)
    xq = xq / xq.norm(dim=1, keepdim=True).clamp_min(1e-12)
    sim, idx = torch.topk(xq @ xb.T, K, dim=1)
    return {"idx": idx}


def same_lists(a, b):
    return float((a.long().cpu() == b.long().cpu()).all(dim=1).float().mean())


result = {"n": N, "F": F, "K": K, "reps": reps}
for tag, q_rows in (("all", test_dev), ("few", test_dev[:FEW].contiguous())):
    n_q, n_b = int(q_rows.numel()), int(train_dev.numel())
    splits = knn.load_knn_library().hipac_knn_bank_splits(n_q, n_b, F, K)
    qs, bs = knn.inv_norms(X, q_rows), knn.inv_norms(X, train_dev)
    fns = {"device probe": lambda: device_probe(q_rows), "device search": lambda: device_search(q_rows, qs, bs),
           "torch mm + topk": lambda: torch_probe(q_rows)}
    counts = {k: reps for k in fns}
    sub = test[:min(host_queries, n_q)]
    if not no_host:
        fns["host float64, 16 threads"] = lambda: host_probe(sub)
        counts["host float64, 16 threads"] = host_reps
    ms, last = alternate(fns, counts)
    flop = 2.0 * n_q * n_b * F
    rate = flop / (ms["device search"] * 1e-3)
    eq_torch = same_lists(last["device probe"]["idx"], last["torch mm + topk"]["idx"])
    pred_eq = float((last["device probe"]["pred"].cpu() == last["torch mm + topk"]["pred"].cpu()).float().mean())
    acc = float((last["device probe"]["pred"].cpu().numpy() == y[test[:n_q]]).mean())
    print(f"-- {n_q} queries x {n_b} bank rows ({splits} column group(s)):")
    print(f"   probe end to end: device {ms['device probe']:.1f} ms; torch mm + topk {ms['torch mm + topk']:.1f} ms "
          f"({ms['torch mm + topk'] / ms['device probe']:.2f} x)")
    print(f"   search alone {ms['device search']:.1f} ms: {rate / 1e12:.1f} TFLOP/s executed = {rate / MFMA_F32_PEAK:.2f} of the exact-f32 MFMA peak")
    print(f"   lists equal to torch's: {eq_torch:.4f} of the queries; predictions equal: {pred_eq:.4f}; accuracy {acc:.4f}")
    r = {"n_q": n_q, "n_b": n_b, "splits": splits, "device_probe_ms": ms["device probe"], "device_search_ms": ms["device search"],
         "torch_ms": ms["torch mm + topk"], "tflops": rate / 1e12, "share_of_peak": rate / MFMA_F32_PEAK, "lists_equal_torch": eq_torch}
    if not no_host:
        scaled = ms["host float64, 16 threads"] * n_q / sub.size
        eq_host = same_lists(last["device probe"]["idx"][:sub.size], last["host float64, 16 threads"]["idx"])
        print(f"   host float64, 16 threads: {ms['host float64, 16 threads']:.0f} ms for {sub.size} queries = {scaled:.0f} ms scaled to all "
              f"({scaled / ms['device probe']:.0f} x); lists equal to float64's: {eq_host:.4f} of {sub.size}")
        r.update(host_ms_scaled=scaled, host_queries=int(sub.size), lists_equal_float64=eq_host)
    result[tag] = r
print(json.dumps(result))
