"""Developer tool (GPU box): the bootstrap of --run_evaluation (froc_ci.py, csrc/eval_ci.hip, --eval_bootstrap) against the
host composition it is defined by -- froc.computeFROC + froc.froc_score on the resampled case lists and the double-loop
AUC (tests/eval_ci_cpu.composition), one host thread -- on two synthetic tables: 129 cases x 2 000 detections (a test
set at --detect_max 2000) and 300 x 240, B = 2 000 replicates.
  * device: build_tables + hipac_eval_ci_bootstrap + finish + the percentiles, i.e. everything between the case lists and
    bootstrap_results.json, uploads and the copy back included;
  * host: the composition of `host_reps` replicates (their counts drawn beforehand), scaled to B -- the replicates are
    independent, so the scaling is linear; all B would take minutes per run.
Medians of 7 runs after a warm-up, the device synchronised on both sides of every timed region, the two modes alternated
run by run.  It also holds the device's replicates against the host's, bit for bit.  Not a gate.
usage: python tools/evalcibench.py [B] [host_reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_ci_cpu as ref  # noqa: E402
from ss25_hierarchical_multiscale_image_classification_amd import froc, froc_ci  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
host_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
RUNS, SEED = 7, 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(ts):
    return sorted(ts)[len(ts) // 2]


for S, per_case in ((129, 2000), (300, 240)):
    t = ref.random_table(20 + S, S, S * per_case)
    fps, sens = froc.computeFROC(ref.froc_data(t))
    point = {"froc_score": froc.froc_score(fps, sens), "sensitivity_at": froc_ci.sensitivity_at(fps, sens),
             "auc": froc_ci.roc_curve(t["labels"], t["scores"])[3]}
    counts = ref.draws(SEED, 0, host_reps, S)

    def device():
        tables = froc_ci.build_tables(ref.froc_data(t), t["scores"], t["labels"])
        fin = froc_ci.finish(froc_ci.bootstrap_integers(tables, SEED, 0, B))
        return fin, froc_ci.bootstrap_results(fin, point, B, SEED, 95.0, True)

    def kernel_only(tables):
        return froc_ci.bootstrap_integers(tables, SEED, 0, B)

    def host():
        return [ref.composition(t, c) for c in counts]

    tables = froc_ci.build_tables(ref.froc_data(t), t["scores"], t["labels"])
    timed(device), timed(host), timed(lambda: kernel_only(tables))
    ts = {"device": [], "host": [], "kernel": []}
    for _ in range(RUNS):
        ms, (fin, res) = timed(device)
        ts["device"].append(ms)
        ms, comp = timed(host)
        ts["host"].append(ms)
        ts["kernel"].append(timed(lambda: kernel_only(tables))[0])
    equal = all(np.array_equal(fin["sensitivity_at"][r], six, equal_nan=True) and np.array_equal(fin["froc_score"][r], score, equal_nan=True)
                and np.array_equal(fin["auc"][r], auc, equal_nan=True) for r, (six, score, auc) in enumerate(comp))
    dev, hst = median(ts["device"]), median(ts["host"]) * B / host_reps
    print(f"{S} cases x {per_case} detections ({tables['ev_case'].shape[0]} events, {tables['n_thresholds']} thresholds), B = {B}: "
          f"device {dev:.1f} ms (upload + kernel + copy back alone {median(ts['kernel']):.1f} ms), host composition "
          f"{hst / 1e3:.1f} s ({median(ts['host']) / host_reps:.1f} ms per replicate over {host_reps}, scaled to B), ratio {hst / dev:.0f}x; "
          f"first {host_reps} replicates equal bit for bit: {equal}; score {res['froc_score']['value']:.4f} "
          f"[{res['froc_score']['lo']:.4f}, {res['froc_score']['hi']:.4f}], AUC {res['auc']['value']:.4f} [{res['auc']['lo']:.4f}, {res['auc']['hi']:.4f}]")
