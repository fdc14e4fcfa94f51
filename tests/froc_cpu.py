"""A plain restatement of the CAMELYON16 FROC script's arithmetic for the tests (scipy for the evaluation mask; numpy
moments for scikit-image's major axis, which is not installed).  Written for comparison, not speed: the threshold loop
is the quadratic one."""
import numpy as np


def evaluation_mask(mask_u8, resolution=0.243, level=5):
    from scipy import ndimage as nd

    dist = nd.distance_transform_edt(255 - np.asarray(mask_u8, np.uint8))
    binary = dist < 75 / (resolution * pow(2, level) * 2)
    filled = nd.binary_fill_holes(binary)
    labels, _ = nd.label(filled, structure=np.ones((3, 3), bool))
    return labels.astype(np.int32)


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
