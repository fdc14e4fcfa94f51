"""Oracle: the pair modes of the inference trunk (precision fp16x3 and fp16q8; csrc/halo16x2.h, the SPLIT / Q8 forms of
csrc/stem.h, csrc/pool.h) restated CONV BY CONV in torch float64 on the CPU, from the device's RAW operand planes.

TEST INFRASTRUCTURE (see oracle/__init__.py).  tests/test_gpu_resnet*.py hold these modes to 2e-5 (fp16x3) / 1e-4 (fp16q8) of
every map's largest value against the fp32 oracle, end to end.  Everything that separates a pair mode from plain fp16 -- the lo
planes and the two cross products, the e4m3 rows and their fixed scales, the per-conv weight scale 2^S and its undoing, the
residual's lo plane, the LO16 = false first convs of fp16q8, the two ways a byte tensor is made -- lives in terms of about
2^-11 of a conv's sum, and a dropped tap or two exchanged channels in that machinery stay under those gates
(tests/test_oracle_pair_replay.py measures which).  Here every conv is recomputed from the operand planes THE DEVICE STORED
(capi.PackedResNet18.raw_tap: the fp16 pair tensor [pixel][hi: C | lo: C] and, in fp16q8, the e4m3 byte tensor
[pixel][C / 64][lo8: 64 | hi8: 64], copied byte for byte), with the weights restated here from the state dict -- never read
back from the device.  In float64 every product of two such operands is exact, so what is left between the replay and the
device is the order of an fp32 sum; the gate comes from the measured distance of a float32 stand-in, not from a worst case
(the bound (K + 2) e S of oracle/infer_replay.py is wider than every fault listed in tests/pair_replay_cases.py).
Pinned on the oracle and on single faults by tests/test_oracle_pair_replay.py, run against the device by
tests/test_gpu_pair_replay.py.  oracle/infer_replay.py does the same for bf16 / fp16 / fp32, block by block, with derived
worst-case bounds: there one ROUNDING lies between input and output, here a dozen bits more are at stake.

Weights (csrc/resnet_pack.hip: pack_conv_pairs, pack_net, the pair branch of pack_stem_u8), restated in ``pack``:
    scale = gamma / sqrt((double)var + (double)(float)eps), bias = (float)(beta - mean scale)            (double)
    S     = floor(log2(2^13 / max |w scale|)) clamped to [0, 15]; a folded projection shares its conv's S (the larger maximum)
    v     = (float)(w scale 2^S),  whi = rn16(v),  wlo = rn16(v - whi)
    whi8  = e4m3(whi 2^-5),  wlo8 = e4m3(wlo 2^6)            OCP e4m3, round to nearest even, saturating at +-448
    bias_c2p = (float)b2 + (float)bp, added in float
    stem  w'' = w scale / (255 std_c), S clamped to [0, 24], the same split; the bias table of infer_replay.strip_table over
          whi + wlo and b0 2^S, rounded to float; tab[1024] = 2^-S
One conv, in float64 from the raw input planes (xhi, xlo | lo8, hi8), the residual pair (rhi, rlo) or the projection's raw input:
    fp16x3   acc = sum xhi whi + sum xhi wlo + sum xlo whi
    fp16q8   acc = sum xhi whi + 2^-6 sum (lo8 whi8 + hi8 wlo8)
    both     + 2^S (rhi + rlo)   or the projection's three (two-kind) sums over its input;   ref = relu(acc 2^-S + bias)
Tolerance  b = FACTOR d_conv max|ref|,  FACTOR = 10 (the rule of tests/test_gpu_train_stages.py), d_conv the largest
max|v - ref| / max|ref| the float32 stand-in's unrounded epilogue value v leaves at that conv
(tests/golden/pair_replay_distances.json, written by tests/tools/measure_pair_replay.py).  Per element, none left out:
    sum     |hi + lo - ref| <= b + 2^-22 |ref|      an output with a lo plane; the fp32 last map (there lo = 0)
    rms     the same maps: sqrt(mean (hi + lo - ref)^2) over every channel, every row and every column of the map, each KIND of
            slice against its own gate FACTOR d_rms[kind] max|ref|, d_rms[kind] the stand-in's largest such figure at that
            conv.  The largest element of an fp32 sum's error is 4 - 5 times its root mean square, while a fault along a border
            or in one chunk is coherent over a slice; and a row or column of the map (thousands of elements) has a far
            steadier root mean square than one channel of a 7 x 7 map (49 elements: 3.2e-7 against a column's 8.2e-8 on the
            last map), so one figure for all three kinds would leave the column gate four times too wide.  It matters on the
            fp32 last map, which has no rounding interval to fall out of (tests/test_oracle_pair_replay.py: a dropped tap at
            output column 0 stands at 2.4 - 2.6 of the element-wise gate there and at 6.7 of the column gate).
    hi      hi in [rn16(ref - b), rn16(ref + b)]
    lo      lo in [rn16(l' - b), rn16(l' + b)],  l' = ref - hi_dev
    pair    hi == rn16(hi + lo) up to an exact tie, |lo| <= ulp(hi) / 2
    hi8     epilogue bytes (made from the unrounded v, l: halo16x2.h, the direct epilogue):
            hi8 in [e4m3(min(max(ref - b, 0), 448)), e4m3(min(ref + b, 448))]
    lo8     lo8 in [e4m3(clamp((l' - b) 2^11)), e4m3(clamp((l' + b) 2^11))]       both by the conversions' monotonicity
    tie     an output with BOTH a lo plane and epilogue bytes: b is far wider than |l - rn16(l)|, so the interval cannot tell
            lo8 = e4m3(l 2^11) from e4m3(rn16(l) 2^11).  The stored lo16 can: where lo16 2^11 lies EXACTLY between two e4m3
            values (T elements) a byte made from lo16 follows ties-to-even always; a byte made from the unrounded l goes the
            other way whenever l lies on the other side of lo16.  l = v - hi is a multiple of v's last place with up to 13
            significant bits (24 of v less the 11 of hi): with 13, the two bits lo16 dropped are 01, 10 or 11 three times in
            four and half of those point away from the even neighbour (3 / 8); with 12 (a quarter of all l) 1 / 4; with
            fewer, or where lo16 is an fp16 subnormal, l = lo16 and nothing differs: about a quarter of T at most, and the
            float32 stand-in, which does the epilogue's arithmetic operation by operation, has 0.15 - 0.21 of T
            (tests/golden/pair_replay_distances.json, "tie_rate").  Asserted: the bytes that differ from e4m3(lo16 2^11), m,
            number at least T / 16 (ratio = T / (16 m); evaluated where T >= 600: T / 16 then lies 6 standard deviations
            below 0.15 T) and at least 1 where 100 <= T < 600 (a rate of 0.15 leaves none with probability 0.85^100 < 1e-7),
            and every difference sits on such a tie.
    bytes   a byte tensor made from the STORED halves (pairs_to_q8_kernel: the pooled map of the unfused stem; the strip
            stem's Q8 form converts its staged halves): byte for byte e4m3(hi), e4m3(lo 2^11)
An fp16q8 inner map (LO16 = false: nothing writes its lo plane, nothing reads it) takes hi, hi8 and lo8 only.
Stem + pool: the strip kernel from the uint8 batch, (whi + wlo)(v - 128) on top of the class table, max over the 3 x 3 / 2
window, ReLU, times tab[1024]; the unfused form (HIPAC_STEM_STRIP=0) from the float input on the exact f32 stem.  Head:
infer_replay.check_head on the fp32 last map.

Every stage returns a dict: ``ratio`` (ASSERTED <= 1: the worst of the checks above), ``dist`` = the plain
max|dev - ref| / max|ref| (dev = hi + lo; an fp16q8 inner map: hi + lo8 2^-11), ``n_out``, ``worst`` and ``checks`` = the
worst ratio per check.  Maps are NCHW float64 tensors; a map's planes travel as a dict {"hi", "lo", "hi8", "lo8"} or {"f32"}.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from . import infer_replay as IR
from .resnet18_ref import BN_EPS
from .transform_ref import IMAGENET_STD

MODES = ("fp16x3", "fp16q8")
FACTOR = 10.0
BLOCKS = IR.BLOCKS
CONVS = tuple(f"{b}.conv{k}" for b in BLOCKS for k in (1, 2))
LO_SHIFT, WHI_SHIFT, WLO_SHIFT = 11, -5, 6  # csrc/common.h: kQ8LoShift, kQ8WhiShift, kQ8WloShift
H16, F8 = torch.float16, torch.float8_e4m3fn
INF = float("inf")


def rn16(t: torch.Tensor) -> torch.Tensor:
    """RNE to fp16 through float32 (monotone, which is all the intervals need; exact on float32 values)."""
    return t.to(torch.float32).to(H16).to(torch.float64)


def e4m3_bytes(t: torch.Tensor) -> torch.Tensor:
    """The e4m3 byte of clamp(t, +-448), uint8."""
    return t.to(torch.float32).clamp(-448.0, 448.0).to(F8).view(torch.uint8)


def e4m3(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).clamp(-448.0, 448.0).to(F8).to(torch.float64)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# raw planes
# ---------------------------------------------------------------------------------------------------------------------
def decode_pairs(raw: torch.Tensor) -> Dict[str, torch.Tensor]:
    """uint8 [n,H,H,4C], the stored pair tensor [pixel][hi: C | lo: C] -> {"hi", "lo"} NCHW float64."""
    t = raw.contiguous().view(H16)
    C = t.shape[-1] // 2
    return {"hi": t[..., :C].permute(0, 3, 1, 2).to(torch.float64), "lo": t[..., C:].permute(0, 3, 1, 2).to(torch.float64)}


def decode_q8(raw: torch.Tensor) -> Dict[str, torch.Tensor]:
    """uint8 [n,H,H,2C], the stored byte tensor [pixel][C / 64][lo8: 64 | hi8: 64] -> {"lo8", "hi8"} NCHW float64 (the decoded
    e4m3 values; a NaN byte stays NaN and fails every comparison)."""
    n, h, _, c2 = raw.shape
    t = raw.contiguous().view(F8).to(torch.float64).view(n, h, h, c2 // 128, 2, 64)
    pl = lambda k: t[..., k, :].reshape(n, h, h, c2 // 2).permute(0, 3, 1, 2)  # noqa: E731
    return {"lo8": pl(0), "hi8": pl(1)}


def decode_f32(raw: torch.Tensor) -> Dict[str, torch.Tensor]:
    """uint8 [n,7,7,2048], the fp32 last map float[pixel][512] -> {"f32"} NCHW float64."""
    return {"f32": raw.contiguous().view(torch.float32).permute(0, 3, 1, 2).to(torch.float64)}


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------
def _fold_bn(sd, conv: str, bn: str, eps: float):
    e = float(torch.tensor(eps, dtype=torch.float32))  # eps crosses the ABI as a float
    scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + e)
    return sd[conv + ".weight"].double() * scale.view(-1, 1, 1, 1), sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * scale


def pair_shift(wmax: float, cap: int = 15) -> int:
    if not (wmax > 0.0) or not math.isfinite(wmax):
        return 0
    return min(max(math.floor(math.log2(8192.0 / wmax)), 0), cap)


def split(v: torch.Tensor):
    """(float)v -> (rn16(v), rn16(v - hi)), float64 tensors; v - hi is exact in float32."""
    v = v.to(torch.float32)
    hi = v.to(H16).to(torch.float32)
    return hi.to(torch.float64), (v - hi).to(H16).to(torch.float64)


def _pack_conv(w: torch.Tensor, b: torch.Tensor, S: int) -> dict:
    whi, wlo = split(torch.ldexp(w, torch.tensor(S)))
    return dict(S=S, whi=whi, wlo=wlo, whi8=e4m3(whi * 2.0 ** WHI_SHIFT), wlo8=e4m3(wlo * 2.0 ** WLO_SHIFT), bias=_f32(b))


def pack(sd: Dict[str, torch.Tensor], eps: float = BN_EPS) -> dict:
    """The pair modes' weights as float64 tensors: {"stem_u8": {whi, wlo, tab, S}, "stem": {w, b}, "layerS.B": {"conv1",
    "conv2"[, "proj", "S_proj_own"]}, "fc"}; a conv: {S, whi, wlo, whi8, wlo8, bias} -- conv2 of a projection block carries
    bias_c2p as its bias, "proj" the shared S."""
    out: dict = {}
    w, b = _fold_bn(sd, "conv1", "bn1", eps)
    out["stem"] = dict(w=_f32(w), b=_f32(b))
    v = w / (255.0 * torch.tensor(IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1))
    S = pair_shift(float(v.abs().max()), 24)
    whi, wlo = split(v * 2.0 ** S)
    out["stem_u8"] = dict(S=S, whi=whi, wlo=wlo, tab=_f32(IR.strip_table(whi + wlo, b * 2.0 ** S)))
    for name in BLOCKS:
        w1, b1 = _fold_bn(sd, name + ".conv1", name + ".bn1", eps)
        w2, b2 = _fold_bn(sd, name + ".conv2", name + ".bn2", eps)
        blk = dict(conv1=_pack_conv(w1, b1, pair_shift(float(w1.abs().max()))))
        if (name + ".downsample.0.weight") in sd:
            wp, bp = _fold_bn(sd, name + ".downsample.0", name + ".downsample.1", eps)
            S2 = pair_shift(max(float(w2.abs().max()), float(wp.abs().max())))
            blk["conv2"] = dict(_pack_conv(w2, b2, S2), bias=_f32(_f32(b2) + _f32(bp)))
            blk["proj"] = _pack_conv(wp, bp, S2)
            blk["S_proj_own"] = pair_shift(float(wp.abs().max()))
        else:
            blk["conv2"] = _pack_conv(w2, b2, pair_shift(float(w2.abs().max())))
        out[name] = blk
    if "fc.weight" in sd:
        out["fc"] = dict(w=sd["fc.weight"].double(), b=sd["fc.bias"].double())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one conv
# ---------------------------------------------------------------------------------------------------------------------
def _products(mode: str, x: dict, wt: dict, stride: int, pad: int) -> torch.Tensor:
    c = lambda a, w: F.conv2d(a, w, None, stride=stride, padding=pad)  # noqa: E731
    if mode == "fp16x3":
        return c(x["hi"], wt["whi"] + wt["wlo"]) + c(x["lo"], wt["whi"])  # (whi + wlo is exact in float64)
    return c(x["hi"], wt["whi"]) + 2.0 ** -WLO_SHIFT * (c(x["lo8"], wt["whi8"]) + c(x["hi8"], wt["wlo8"]))


def conv_ref(mode: str, x: dict, wt: dict, stride: int = 1, resid: Optional[dict] = None, proj_x: Optional[dict] = None,
             proj_w: Optional[dict] = None) -> torch.Tensor:
    """relu(acc 2^-S + bias) of the module docstring, float64 NCHW."""
    acc = _products(mode, x, wt, stride, 1)
    if resid is not None:
        acc = acc + 2.0 ** wt["S"] * (resid["hi"] + resid["lo"])
    if proj_x is not None:
        acc = acc + _products(mode, proj_x, proj_w, 2, 0)
    return (acc * 2.0 ** -wt["S"] + wt["bias"].view(1, -1, 1, 1)).clamp_min(0)


def _ivl(dev: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """|dev - middle| / half-width per element; an element outside an interval of width 0 gives inf, a NaN gives inf."""
    half, mid = (hi - lo) / 2, (hi + lo) / 2
    inside = (dev >= lo) & (dev <= hi)
    r = torch.where(half > 0, (dev - mid).abs() / half.clamp_min(1e-300), torch.where(inside, 0.0, INF).to(dev.dtype)).nan_to_num(nan=INF, posinf=INF)
    return torch.where(inside, r.clamp_max(1.0), r.clamp_min(math.nextafter(1.0, 2.0)))


def pair_faults(p: dict) -> torch.Tensor:
    """0 / inf per element: hi == rn16(hi + lo) up to an exact tie, and |lo| <= half a unit in the last place of hi."""
    hi, lo = p["hi"], p["lo"]
    s = hi + lo  # exact
    r = rn16(s)
    bad = ((r != hi) & ((s - r).abs() != (s - hi).abs())) | (lo.abs() > IR._cell_half(hi, H16)) | ~torch.isfinite(s)
    return torch.where(bad, torch.full_like(s, INF), torch.zeros_like(s))


def stored_bytes_faults(p: dict) -> torch.Tensor:
    """0 / inf per element: the byte planes equal, byte for byte, e4m3(hi) and e4m3(lo 2^11) of the STORED halves."""
    bad = (e4m3_bytes(p["hi"]) != e4m3_bytes(p["hi8"])) | (e4m3_bytes(p["lo"] * 2.0 ** LO_SHIFT) != e4m3_bytes(p["lo8"]))
    bad |= torch.isnan(p["hi8"]) | torch.isnan(p["lo8"])
    return torch.where(bad, torch.full_like(p["hi"], INF), torch.zeros_like(p["hi"]))


TIE_MIN, TIE_ANY = 600, 100


def tie_statistic(p: dict) -> Dict[str, float]:
    """The ``tie`` check of the module docstring on an output with a lo plane and epilogue bytes."""
    lo_s = p["lo"] * 2.0 ** LO_SHIFT
    q = e4m3(lo_s)
    # exactly between two e4m3 values: stepping the byte one place away from zero / towards zero gives a value as far away
    b = e4m3_bytes(lo_s).to(torch.int16)
    mag = b & 0x7F
    other = lambda m: torch.where(b >= 128, m + 128, m).to(torch.uint8).view(F8).to(torch.float64)  # noqa: E731
    up, dn = other((mag + 1).clamp_max(0x7E)), other((mag - 1).clamp_min(0))
    err = (lo_s - q).abs()
    on_tie = (err > 0) & (((up - lo_s).abs() == err) | ((dn - lo_s).abs() == err)) & (lo_s.abs() < 448.0)
    differs = p["lo8"] != q
    T, m, stray = int(on_tie.sum()), int((differs & on_tie).sum()), int((differs & ~on_tie).sum())
    ratio = (INF if m == 0 else T / (16.0 * m)) if T >= TIE_MIN else (INF if m == 0 and T >= TIE_ANY else 0.0)
    return dict(T=T, m=m, stray=stray, ratio=INF if stray else ratio)


RMS_KINDS = {"ch": (2, 3), "row": (1, 3), "col": (1, 2)}  # a slice kind -> the dimensions of [n,C,H,W] it averages over


def slice_rms(err: torch.Tensor) -> Dict[str, float]:
    """Per slice kind, the largest root mean square of ``err`` [n,C,H,W] over one channel, one row or one column of one image."""
    sq = err * err
    return {k: float(sq.mean(dim=dims).max().sqrt()) for k, dims in RMS_KINDS.items()}


def _rms_ratios(err: torch.Tensor, d_rms: Dict[str, float], absmax: float) -> Dict[str, float]:
    got = slice_rms(err.nan_to_num(nan=INF, posinf=INF))
    return {"rms_" + k: got[k] / max(FACTOR * d_rms[k] * absmax, 1e-300) for k in RMS_KINDS}


def _result(ref: torch.Tensor, dev_v: torch.Tensor, checks: Dict[str, torch.Tensor], extra: Optional[Dict[str, float]] = None) -> dict:
    r = torch.stack([c.expand_as(ref) for c in checks.values()]).max(dim=0).values
    per = {k: float(c.max()) for k, c in checks.items()}
    per.update(extra or {})
    worst = tuple(int(i) for i in torch.unravel_index(torch.argmax(r), r.shape))
    return dict(ratio=max(per.values()), dist=float((dev_v - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
                n_out=int((r > 1.0).sum()), worst=worst, checks=per, absmax=float(ref.abs().max()))


def check_map(ref: torch.Tensor, out: dict, d: float, d_rms: Dict[str, float], mode: str, lo16: bool = True, bytes_from: Optional[str] = None) -> dict:
    """Every per-element check of the module docstring on one map ``out`` against its float64 ``ref``.  ``lo16``: the map has a
    lo plane; ``bytes_from``: None (no byte tensor), "epilogue" or "stored"."""
    b = FACTOR * d * float(ref.abs().max())
    absmax = float(ref.abs().max())
    checks: Dict[str, torch.Tensor] = {}
    extra: Dict[str, float] = {}
    if "f32" in out:
        v = out["f32"]
        checks["sum"] = (v - ref).abs() / (b + 2.0 ** -22 * ref.abs()).clamp_min(1e-300)
        checks["sum"] = checks["sum"].nan_to_num(nan=INF, posinf=INF)
        return _result(ref, v, checks, _rms_ratios(v - ref, d_rms, absmax))
    hi = out["hi"]
    checks["hi"] = _ivl(hi, rn16(ref - b), rn16(ref + b))
    lp = ref - hi
    v = hi
    if lo16:
        v = hi + out["lo"]
        checks["sum"] = ((v - ref).abs() / (b + 2.0 ** -22 * ref.abs()).clamp_min(1e-300)).nan_to_num(nan=INF, posinf=INF)
        checks["lo"] = _ivl(out["lo"], rn16(lp - b), rn16(lp + b))
        checks["pair"] = pair_faults(out)
        extra.update(_rms_ratios(v - ref, d_rms, absmax))
    if bytes_from == "epilogue":
        checks["hi8"] = _ivl(out["hi8"], e4m3((ref - b).clamp(0.0, 448.0)), e4m3((ref + b).clamp_max(448.0)))
        sc = 2.0 ** LO_SHIFT
        checks["lo8"] = _ivl(out["lo8"], e4m3(((lp - b) * sc).clamp(-448.0, 448.0)), e4m3(((lp + b) * sc).clamp(-448.0, 448.0)))
        if lo16:
            t = tie_statistic(out)
            extra["tie"] = t["ratio"]
        else:
            v = hi + out["lo8"] * 2.0 ** -LO_SHIFT
    elif bytes_from == "stored":
        checks["bytes"] = stored_bytes_faults(out)
    res = _result(ref, v, checks, extra)
    if "tie" in extra:
        res["tie"] = t
    return res


# ---------------------------------------------------------------------------------------------------------------------
# stem + pool, head
# ---------------------------------------------------------------------------------------------------------------------
def stem_pool_ref(form: str, inp: torch.Tensor, W: dict) -> torch.Tensor:
    """The pooled map [n,64,56,56] in float64.  "u8_strip": uint8 [n,224,224,3]; "nchw_f32" (the unfused form, which the
    device also takes for uint8 input with HIPAC_STEM_STRIP=0 after its fp32 table): float [n,3,224,224]."""
    if form == "u8_strip":
        st = W["stem_u8"]
        c = F.pad(inp.permute(0, 3, 1, 2).to(torch.float64) - 128.0, (3, 3, 3, 3), value=-128.0)  # bytes outside arrive as 0
        cls = torch.zeros(112, dtype=torch.long)
        cls[0], cls[1], cls[111] = 1, 2, 3
        t = st["tab"][cls][:, cls].permute(2, 0, 1).unsqueeze(0)
        a = F.conv2d(c, st["whi"] + st["wlo"], None, stride=2) + t
        return IR._max_pool(a.clamp_min(0)) * 2.0 ** -st["S"]
    if form != "nchw_f32":
        raise ValueError(form)
    a = F.conv2d(_f32(inp), W["stem"]["w"], None, stride=2, padding=3) + W["stem"]["b"].view(1, -1, 1, 1)
    return IR._max_pool(a.clamp_min(0))


def check_stem_pool(mode: str, form: str, inp, W: dict, pool: dict, d: float, d_rms: Dict[str, float]) -> dict:
    """The pooled pair tensor (and fp16q8's bytes, made from the stored halves in both forms) against ``stem_pool_ref``."""
    return check_map(stem_pool_ref(form, inp, W), pool, d, d_rms, mode, True, "stored" if mode == "fp16q8" else None)


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
def conv_plan(i: int) -> dict:
    """Block i: the stride of its first conv and whether its shortcut is the folded projection."""
    down = i in (2, 4, 6)
    return dict(stride=2 if down else 1, proj=down)


def check_forward(mode: str, dev: dict, W: dict, dist: Dict[str, float], stem: str = "u8_strip", pool_head: bool = True,
                  head: bool = True) -> Dict[str, dict]:
    """Every stage of one forward from the device's own planes.  ``dev``: "input", "pool", "inner" [8], "out" [8] (planes
    dicts; out[7] = {"f32"}), "feats", optional "logits".  ``dist``: the mode's entry of the JSON, {"max": d per stage, "rms": {slice kind: d_rms} per stage}.  -> {stage:
    figures}: "stem_pool", the 16 convs, and with ``head`` "feats", "logits"."""
    q8 = mode == "fp16q8"
    eb = "epilogue" if q8 else None
    res = {"stem_pool": check_stem_pool(mode, stem, dev["input"], W, dev["pool"], dist["max"]["stem_pool_" + stem], dist["rms"]["stem_pool_" + stem])}
    X = dev["pool"]
    for i, name in enumerate(BLOCKS):
        w, pl = W[name], conv_plan(i)
        ref1 = conv_ref(mode, X, w["conv1"], pl["stride"])
        res[name + ".conv1"] = check_map(ref1, dev["inner"][i], dist["max"][name + ".conv1"], dist["rms"][name + ".conv1"], mode, lo16=not q8, bytes_from=eb)
        if pl["proj"]:
            ref2 = conv_ref(mode, dev["inner"][i], w["conv2"], 1, proj_x=X, proj_w=w["proj"])
        else:
            ref2 = conv_ref(mode, dev["inner"][i], w["conv2"], 1, resid=X)
        res[name + ".conv2"] = check_map(ref2, dev["out"][i], dist["max"][name + ".conv2"], dist["rms"][name + ".conv2"], mode, lo16=True, bytes_from=None if i == 7 else eb)
        X = dev["out"][i]
    if head:
        res.update(IR.check_head(dev["out"][7]["f32"], dev["feats"], dev.get("logits"), W.get("fc"), pool_head))
    return res


def slice_image(dev: dict, i: int) -> dict:
    def sl(v):
        if isinstance(v, dict):
            return {k: sl(t) for k, t in v.items()}
        if isinstance(v, (list, tuple)):
            return [sl(t) for t in v]
        return v[i:i + 1]
    return {k: sl(v) for k, v in dev.items() if v is not None}


def check_images(mode: str, dev: dict, images: Sequence[int], W: dict, dist: Dict[str, float], **forms) -> Dict[str, dict]:
    """``check_forward`` image by image over ``images`` of the batch ``dev`` holds; per stage the worst image's figures (n_out
    summed, dist and every check's ratio the largest, "tie" the image with the lowest rate), its "worst" index led by the image's number."""
    merged: Dict[str, dict] = {}
    for i in images:
        for stage, r in check_forward(mode, slice_image(dev, i), W, dist, **forms).items():
            r = dict(r, worst=(i,) + tuple(r["worst"][1:]))
            m = merged.get(stage)
            if m is None:
                merged[stage] = r
                continue
            best = dict(r if r["ratio"] > m["ratio"] else m)
            best["n_out"] = m["n_out"] + r["n_out"]
            for k in ("dist", "fig", "sqrtk"):
                if k in r:
                    best[k] = max(m[k], r[k])
            if "checks" in r:
                best["checks"] = {k: max(m["checks"][k], r["checks"][k]) for k in r["checks"]}
            if "tie" in r:  # the image with the lowest rate m / T among those the check was evaluated on
                rate = lambda t: t["m"] / t["T"] if t["T"] >= TIE_ANY else INF  # noqa: E731
                best["tie"] = r["tie"] if rate(r["tie"]) < rate(m["tie"]) else m["tie"]
            merged[stage] = best
    return merged


def summary(results: Dict[str, dict]) -> str:
    lines = []
    for s, r in results.items():
        if "checks" in r:
            ck = " ".join(f"{k} {v:.3g}" for k, v in r["checks"].items())
            tie = f"  ties {r['tie']['m']}/{r['tie']['T']}" if "tie" in r else ""
            lines.append(f"  {s:15s} ratio {r['ratio']:.3g}  dist {r['dist']:.3g}  outside {r['n_out']}  worst {r['worst']}  [{ck}]{tie}")
        else:
            lines.append(f"  {s:15s} ratio {r['ratio']:.3g}  fig {r['fig']:.3g}  outside {r['n_out']}  worst {r['worst']}")
    return "\n".join(lines)


def failures(results: Dict[str, dict]) -> List[str]:
    return [f"{s}: ratio {r['ratio']:.3g}, {r['n_out']} elements outside, worst at (image, channel, row, column) = {r['worst']}"
            + (f", checks {r['checks']}" if "checks" in r else "") for s, r in results.items() if not r["ratio"] <= 1.0]
