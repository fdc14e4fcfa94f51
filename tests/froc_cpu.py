"""A plain restatement of the CAMELYON16 FROC script's arithmetic for the tests (scipy for the evaluation mask; numpy
moments for scikit-image's major axis, which is not installed).  Written for comparison, not speed: the threshold loop
is the quadratic one.  ``evaluation_mask_pure`` is the evaluation mask again without scipy (brute-force distances and
flood fills), pinned to scipy's recorded labels by tests/test_froc_reference.py."""
import math

import numpy as np


def evaluation_mask(mask_u8, resolution=0.243, level=5):
    from scipy import ndimage as nd

    dist = nd.distance_transform_edt(255 - np.asarray(mask_u8, np.uint8))
    binary = dist < 75 / (resolution * pow(2, level) * 2)
    filled = nd.binary_fill_holes(binary)
    labels, _ = nd.label(filled, structure=np.ones((3, 3), bool))
    return labels.astype(np.int32)


def threshold_k(resolution=0.243, level=5):
    """The least integer K with sqrt(float(K)) >= T: for an integer squared distance, sqrt(d2) < T is d2 < K."""
    T = 75 / (resolution * pow(2, level) * 2)
    K = int(math.ceil(T * T))
    while K > 0 and math.sqrt(float(K - 1)) >= T:
        K -= 1
    while math.sqrt(float(K)) < T:
        K += 1
    return K


def _binary_brute_force(m, K):
    """(exact squared distance to the nearest byte == 255) < K, with no separable pass: the minimum over the seed list,
    or the OR of the seed image shifted by every offset with dr^2 + dc^2 < K, whichever touches fewer pixels."""
    H, W = m.shape
    seed = m == 255
    rows, cols = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
    if not seed.any():  # scipy's virtual zero at (row -1, column 0)
        return ((rows + 1) ** 2)[:, None] + (cols ** 2)[None, :] < K
    R = math.isqrt(K - 1)  # the largest g with g * g < K
    offsets = [(dr, dc) for dr in range(-min(R, H - 1), min(R, H - 1) + 1) for dc in range(-min(R, W - 1), min(R, W - 1) + 1)
               if dr * dr + dc * dc < K]
    # a seed between four seeds is never the nearest seed of a pixel that is not a seed itself
    inner = np.zeros_like(seed)
    inner[1:-1, 1:-1] = seed[1:-1, 1:-1] & seed[:-2, 1:-1] & seed[2:, 1:-1] & seed[1:-1, :-2] & seed[1:-1, 2:]
    edge = np.argwhere(seed & ~inner)
    if len(edge) <= len(offsets):
        d2 = np.full((H, W), np.iinfo(np.int64).max, np.int64)
        for sr, sc in edge:
            np.minimum(d2, ((rows - sr) ** 2)[:, None] + ((cols - sc) ** 2)[None, :], out=d2)
        return (d2 < K) | seed
    out = np.zeros((H, W), bool)
    for dr, dc in offsets:  # out[r, c] |= seed[r + dr, c + dc]
        r0, r1, c0, c1 = max(0, -dr), min(H, H - dr), max(0, -dc), min(W, W - dc)
        out[r0:r1, c0:c1] |= seed[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def _flood(open_, start, steps):
    """Depth-first flood over the flat padded grid ``open_`` (1 = may be entered, cleared on entry); returns the pixels."""
    open_[start] = 0
    stack, seen = [start], [start]
    while stack:
        p = stack.pop()
        for s in steps:
            q = p + s
            if open_[q]:
                open_[q] = 0
                stack.append(q)
                seen.append(q)
    return seen


def evaluation_mask_pure(mask_u8, resolution=0.243, level=5):
    """``evaluation_mask`` with numpy and plain Python only: brute-force thresholded distances, a 4-connected flood of the
    background from the border (what it does not reach is a hole), an 8-connected flood fill numbered in raster order of
    each component's first pixel."""
    m = np.asarray(mask_u8, np.uint8)
    H, W = m.shape
    binary = _binary_brute_force(m, threshold_k(resolution, level))
    P = W + 2  # one pixel of closed padding all round, so that no step leaves the grid
    pad = np.zeros((H + 2, P), np.uint8)
    pad[1:-1, 1:-1] = ~binary
    bg = bytearray(pad.tobytes())
    border = [(r + 1) * P + c + 1 for r in range(H) for c in ((0, W - 1) if 0 < r < H - 1 else range(W))]
    for p in border:
        if bg[p]:
            _flood(bg, p, (-P, -1, 1, P))
    holes = np.frombuffer(bytes(bg), np.uint8).reshape(H + 2, P)[1:-1, 1:-1].astype(bool)
    pad[1:-1, 1:-1] = binary | holes
    fg = bytearray(pad.tobytes())
    labels = np.zeros((H + 2) * P, np.int32)
    n = 0
    for p in np.flatnonzero(pad.ravel()).tolist():  # raster order
        if fg[p]:
            n += 1
            labels[_flood(fg, p, (-P - 1, -P, -P + 1, -1, 1, P - 1, P, P + 1))] = n
    return labels.reshape(H + 2, P)[1:-1, 1:-1].copy()


def major_axes(labels):
    """scikit-image's regionprops major_axis_length of labels 1..max, from float64 central moments."""
    out = []
    for lab in range(1, int(labels.max(initial=0)) + 1):
        r, c = np.nonzero(labels == lab)
        r, c = r.astype(np.float64), c.astype(np.float64)
        dr, dc = r - r.mean(), c - c.mean()
        t = np.array([[(dc * dc).mean(), -(dr * dc).mean()], [-(dr * dc).mean(), (dr * dr).mean()]])
        out.append(4 * np.sqrt(max(np.linalg.eigvalsh(t).max(), 0.0)))
    return out


def itc_list(labels, resolution=0.243, level=5):
    thr = 275 / (resolution * pow(2, level))
    return [i + 1 for i, ax in enumerate(major_axes(labels)) if ax < thr]


def label_at(labels, x, y, level):
    r, c = int(y / pow(2, level)), int(x / pow(2, level))
    if 0 <= r < labels.shape[0] and 0 <= c < labels.shape[1]:
        return int(labels[r, c])
    return 0


def compute_fp_tp(Ycorr, Xcorr, Probs, is_tumor, labels, itc, level):
    max_label = int(np.amax(labels)) if is_tumor else 0
    fps, fp_summary = [], {}
    tps = np.zeros((max_label,), dtype=np.float32)
    det = {}
    for i in range(1, max_label + 1):
        if i not in itc:
            det["Label " + str(i)] = []
    counter = 0
    for i in range(len(Xcorr)):
        hit = label_at(labels, Xcorr[i], Ycorr[i], level) if is_tumor else 0
        if hit == 0:
            fps.append(Probs[i])
            fp_summary["FP " + str(counter)] = [Probs[i], Xcorr[i], Ycorr[i]]
            counter += 1
        elif hit not in itc:
            if Probs[i] > tps[hit - 1]:
                det["Label " + str(hit)] = [Probs[i], Xcorr[i], Ycorr[i]]
                tps[hit - 1] = Probs[i]
    return fps, tps, max_label - len(itc), det, fp_summary


def compute_froc(names, fps, tps, ntum):
    all_fp = [v for lst in fps for v in lst]
    all_tp = [v for lst in tps for v in lst]
    tot_fp, tot_tp = [], []
    for th in sorted(set(all_fp + all_tp))[1:]:
        tot_fp.append((np.asarray(all_fp) >= th).sum())
        tot_tp.append((np.asarray(all_tp) >= th).sum())
    tot_fp.append(0)
    tot_tp.append(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(tot_fp) / float(len(names)), np.asarray(tot_tp) / float(sum(ntum))


def froc_score(total_fps, sens, rates=(0.25, 0.5, 1, 2, 4, 8)):
    vals = []
    for r in rates:
        ok = [s for f, s in zip(total_fps, sens) if f <= r]
        vals.append(max(ok) if ok else 0.0)
    return float(np.mean(vals))
