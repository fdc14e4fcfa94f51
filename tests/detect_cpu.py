"""A plain numpy float32 restatement of the detection stage (include/hipac_detect.h) for the tests: the same operations in
the same order, so every stage after the probabilities must match the device bit for bit.  Written for comparison, not
speed.  ``nms_greedy`` is the literal loop of the header; ``nms_rounds`` is the round form the device runs, kept here so
that the two can be checked against each other without a GPU."""
import numpy as np

WINDOW_L0 = 1792
F32 = np.float32


def probs_f64(logits, tumor_class=1):
    """The float64 formula the device's float32 probabilities are measured against."""
    lg = np.asarray(logits, np.float64)
    return 1.0 / (1.0 + np.exp(lg[:, 1 - tumor_class] - lg[:, tumor_class]))


def gaussian_taps(sigma):
    """float64 taps as scipy's _gaussian_kernel1d makes them (order 0, truncate 4)."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def grid_of(level0_size, cell):
    return -(-int(level0_size[0]) // cell), -(-int(level0_size[1]) // cell)


def level_map(p, meta, level, cell, grid):
    """(map float32[gh, gw], count int32[gh, gw]): every cell adds p over its K x K candidate origins in raster order."""
    gw, gh = grid
    K, stride = WINDOW_L0 // cell, cell >> level
    origin = np.full((gh, gw), -1, np.int64)
    for w, (lv, x, y, _) in enumerate(np.asarray(meta).reshape(-1, 4).tolist()):
        if lv != level or x < 0 or y < 0:
            continue
        cx, cy = x // stride, y // stride
        if cx < gw and cy < gh:
            origin[cy, cx] = w
    out, count = np.zeros((gh, gw), F32), np.zeros((gh, gw), np.int32)
    for j in range(gh):
        for i in range(gw):
            acc, cnt = F32(0), 0
            for oy in range(max(0, j - K + 1), j + 1):
                for ox in range(max(0, i - K + 1), i + 1):
                    w = origin[oy, ox]
                    if w >= 0:
                        acc = F32(acc + F32(p[w]))
                        cnt += 1
            out[j, i] = F32(acc / F32(cnt)) if cnt else F32(0)
            count[j, i] = cnt
    return out, count


def fuse(maps, counts, mode="mean"):
    """Levels in the order given (ascending); only levels with data at a cell take part."""
    maps, counts = np.asarray(maps, F32), np.asarray(counts)
    acc = np.zeros(maps.shape[1:], F32)
    have = np.zeros(maps.shape[1:], np.int32)
    for m, c in zip(maps, counts):
        on = c > 0
        if mode == "max":
            acc = np.where(on & ((have == 0) | (m > acc)), m, acc).astype(F32)
        else:
            acc = np.where(on, (acc + m).astype(F32), acc).astype(F32)
        have = have + on
    if mode == "max":
        return np.where(have > 0, acc, F32(0)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(have > 0, (acc / have.astype(F32)).astype(F32), F32(0)).astype(F32)


def smooth(m, sigma):
    """Rows, then columns; zeros outside; float32 multiply and float32 add, taps -R .. +R in order."""
    m = np.asarray(m, F32)
    if sigma == 0:
        return m
    taps = gaussian_taps(sigma).astype(F32)
    R = (len(taps) - 1) // 2

    def along_x(a):
        h, w = a.shape
        pad = np.zeros((h, w + 2 * R), F32)
        pad[:, R:R + w] = a
        acc = np.zeros((h, w), F32)
        for k in range(-R, R + 1):
            prod = (taps[k + R] * pad[:, R + k:R + k + w]).astype(F32)
            acc = (acc + prod).astype(F32)
        return acc

    return along_x(along_x(m).T.copy()).T.copy()


def _beats(va, a, vb, b):
    return va > vb or (va == vb and a < b)


def nms_greedy(m, radius, threshold, max_detections):
    """The literal greedy loop: (p float32[k], ij int32[k, 2] = (i, j))."""
    m = np.asarray(m, F32)
    gh, gw = m.shape
    live = m >= F32(threshold)  # NaN never is
    jj, ii = np.mgrid[0:gh, 0:gw]
    ps, ijs = [], []
    while len(ps) < max_detections and live.any():
        vals = np.where(live, m, -np.inf)
        c = int(np.argmax(vals))  # the first of equal values in raster order
        j, i = divmod(c, gw)
        ps.append(m[j, i])
        ijs.append((i, j))
        live &= (ii - i) ** 2 + (jj - j) ** 2 > radius * radius
    return np.asarray(ps, F32), np.asarray(ijs, np.int32).reshape(-1, 2)


def nms_rounds(m, radius, threshold, max_detections):
    """The round form: every live cell that beats all live cells of its neighbourhood is selected at once, the selected
    cells' neighbourhoods are cleared, until nothing is left; then sort by (value descending, index ascending)."""
    m = np.asarray(m, F32)
    gh, gw = m.shape
    live = m >= F32(threshold)
    offs = [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)
            if dx * dx + dy * dy <= radius * radius and (dx or dy)]
    chosen, rounds = [], 0
    while live.any():
        rounds += 1
        sel = []
        for c in np.flatnonzero(live).tolist():
            j, i = divmod(c, gw)
            ok = True
            for dx, dy in offs:
                x, y = i + dx, j + dy
                if 0 <= x < gw and 0 <= y < gh and live[y, x] and _beats(m[y, x], y * gw + x, m[j, i], c):
                    ok = False
                    break
            if ok:
                sel.append(c)
        for c in sel:
            j, i = divmod(c, gw)
            live[j, i] = False
            for dx, dy in offs:
                x, y = i + dx, j + dy
                if 0 <= x < gw and 0 <= y < gh:
                    live[y, x] = False
        chosen += sel
    chosen.sort(key=lambda c: (-float(m.flat[c]), c))
    chosen = chosen[:max_detections]
    ps = np.asarray([m.flat[c] for c in chosen], F32)
    ijs = np.asarray([(c % gw, c // gw) for c in chosen], np.int32).reshape(-1, 2)
    return ps, ijs, rounds


def detect(p, meta, level0_size, levels=(0, 1, 2, 3), cell=224, fuse_mode="mean", sigma=1.0, radius=4, threshold=0.5,
           max_detections=2000):
    """The whole stage from the probability vector: a dict with maps, counts, fused, smoothed, prob, ij, x, y."""
    levels = tuple(sorted(levels))
    grid = grid_of(level0_size, cell)
    p = np.asarray(p, F32)
    lm = [level_map(p, meta, l, cell, grid) for l in levels]
    maps, counts = np.stack([a for a, _ in lm]), np.stack([b for _, b in lm])
    fused = fuse(maps, counts, fuse_mode)
    sm = smooth(fused, sigma)
    prob, ij = nms_greedy(sm, radius, threshold, max_detections)
    x = [int((int(i) + 0.5) * cell) for i in ij[:, 0]]
    y = [int((int(j) + 0.5) * cell) for j in ij[:, 1]]
    return {"maps": maps, "counts": counts, "fused": fused, "smoothed": sm, "prob": prob, "ij": ij, "x": x, "y": y}


def csv_text(prob, x, y):
    return "".join(f"{float(p):.9g},{int(a)},{int(b)}\n" for p, a, b in zip(prob, x, y))
