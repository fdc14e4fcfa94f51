"""Cases shared by tests/test_oracle_pair_replay.py (CPU), tests/test_gpu_pair_replay.py and
tests/tools/measure_pair_replay.py, and the CPU STAND-IN of the device's pair modes: the trunk of fp16x3 / fp16q8 with torch
FLOAT32 convolutions of the same operand planes (a summation order that is neither the device's nor the float64 replay's),
the product kinds summed separately and then added, and the epilogue's splits and conversions (oracle/pair_replay.py, module
docstring).  The strip stem is emulated WITHOUT the bias table -- b0 2^S + the sum over the taps inside the image of
(whi + wlo)(v - 255 mean_c) -- so that the table's algebra is checked and not copied.

The stand-in can be built with ONE FAULT, in every conv the fault applies to:
  both    "drop_tap_col0"     centre tap of the xhi * wlo (hi8 * wlo8) product left out at output column 0
          "swap_channels"     two channels of the chunk 32 .. 63 exchanged in wlo (wlo8): the one that carries the most in this
                              conv's input and the one that carries the least (``swap_pair``), so that the exchanged term
                              2^-11 (x_i - x_j)(w_j - w_i) is present at every conv -- with two fixed channels it is no larger
                              than the fp32 sum's own error wherever both happen to carry little
          "resid_hi_only"     the identity shortcut added from the hi plane only
          "winv_proj_own"     a folded-projection conv's accumulator undone with the projection's OWN S (a no-op where the two
                              agree: ``RESCALED_SEED`` makes them differ)
  fp16q8  "scale_m5"          weight-side scale 2^-5 instead of 2^-6
          "lo8_from_lo16"     a block output's lo8 made from the ROUNDED lo16 where the epilogue uses the unrounded l
          "inner_lo8_zero"    an inner map's lo8 all zero (a reader of a plane that was never written)
  fp16x3  "lo_from_hi_band"   the xlo * whi product read from the hi band
"""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

import infer_replay_cases as IC
import rescale_cases
from oracle import pair_replay as PR
from oracle.transform_ref import IMAGENET_MEAN
from ss25_hierarchical_multiscale_image_classification_amd import synth

WEIGHT_SEED = IC.WEIGHT_SEED
RESCALED_SEED = 102  # rescale_cases.rescale_inner(.., 4, seed): found on the CPU (test_rescaled_weights_separate_the_shifts)
FAULTS = {"fp16x3": ("drop_tap_col0", "swap_channels", "resid_hi_only", "winv_proj_own", "lo_from_hi_band"),
          "fp16q8": ("drop_tap_col0", "swap_channels", "resid_hi_only", "winv_proj_own", "scale_m5", "lo8_from_lo16", "inner_lo8_zero")}
patches, normalized = IC.patches, IC.normalized


def state_dict(kind: str = "plain") -> Dict[str, torch.Tensor]:
    sd = synth.seeded_resnet18_state_dict(WEIGHT_SEED, 2)
    return rescale_cases.rescale_inner(sd, 4, seed=RESCALED_SEED) if kind == "rescaled" else sd


def fault_sites(mode: str, fault: str, W: dict):
    """The stages of ``PR.check_forward`` whose conv the fault changes."""
    c1 = [b + ".conv1" for b in PR.BLOCKS]
    c2 = [b + ".conv2" for b in PR.BLOCKS]
    if fault == "resid_hi_only":
        return [c for i, c in enumerate(c2) if not PR.conv_plan(i)["proj"]]
    if fault == "winv_proj_own":
        return [b + ".conv2" for b in PR.BLOCKS if "proj" in W[b] and W[b]["S_proj_own"] != W[b]["conv2"]["S"]]
    if fault == "lo8_from_lo16":
        return c2[:7]
    if fault == "inner_lo8_zero":
        return c1
    return c1 + c2


# ---------------------------------------------------------------------------------------------------------------------
# the float32 stand-in
# ---------------------------------------------------------------------------------------------------------------------
def _f(t):
    return t.to(torch.float32)


def _c(a, w, stride, pad):
    return F.conv2d(a, w, None, stride=stride, padding=pad)


def _e4m3(t):
    return t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32)


def swap_pair(xh: torch.Tensor):
    """The channels of 32 .. 63 with the largest and the smallest mean of the hi-side operand ``xh`` [n,C,H,W]."""
    m = xh[:, 32:64].abs().mean(dim=(0, 2, 3))
    return 32 + int(m.argmax()), 32 + int(m.argmin())


def _products(mode, x, wt, stride, pad, fault):
    """The accumulator's conv sums in float32: hi x hi, then the cross kinds, each its own convolution."""
    xhi, whi = _f(x["hi"]), _f(wt["whi"])
    main = _c(xhi, whi, stride, pad)
    q8 = mode == "fp16q8"
    wl, xh = (_f(wt["wlo8"]), _f(x["hi8"])) if q8 else (_f(wt["wlo"]), xhi)  # the operands of the xhi * wlo product
    if fault == "swap_channels" and pad == 1:
        wl = wl.clone()
        i, j = swap_pair(xh)
        wl[:, [i, j]] = wl[:, [j, i]]
    a = _c(xh, wl, stride, pad)
    if fault == "drop_tap_col0" and pad == 1:
        a[..., 0] -= F.conv2d(xh, wl[:, :, 1:2, 1:2], None, stride=stride)[..., 0]
    if q8:
        cross = a + _c(_f(x["lo8"]), _f(wt["whi8"]), stride, pad)
        return main + cross * (2.0 ** -5 if fault == "scale_m5" else 2.0 ** -6)
    return (main + a) + _c(xhi if fault == "lo_from_hi_band" else _f(x["lo"]), whi, stride, pad)


def standin_conv(mode: str, x: dict, wt: dict, kind: str, stride: int = 1, resid: Optional[dict] = None, proj_x: Optional[dict] = None,
                 proj_w: Optional[dict] = None, S_own: Optional[int] = None, fault: Optional[str] = None) -> dict:
    """One conv of the stand-in -> the planes of its output (float32 tensors of stored values) and "v", the unrounded float32
    epilogue value.  ``kind``: "inner" (a block's first conv: no lo plane in fp16q8 -- NaN here, nothing may read it), "out",
    "last" (the fp32 map)."""
    acc = _products(mode, x, wt, stride, 1, fault)
    S = wt["S"]
    if resid is not None:
        r = _f(resid["hi"]) if fault == "resid_hi_only" else _f(resid["hi"]) + _f(resid["lo"])  # (exact: 22 bits)
        acc = acc + 2.0 ** S * r
    if proj_x is not None:
        acc = acc + _products(mode, proj_x, proj_w, 2, 0, None)
        if fault == "winv_proj_own":
            S = S_own
    u = acc * 2.0 ** -S + _f(wt["bias"]).view(1, -1, 1, 1)  # (the device's one fma: acc 2^-S is exact)
    v = u.clamp_min(0)
    if kind == "last":
        return {"f32": v, "v": v}
    h = v.to(torch.float16).to(torch.float32)
    l = v - h
    lo16 = l.to(torch.float16).to(torch.float32)
    q8 = mode == "fp16q8"
    out = {"hi": h, "lo": torch.full_like(h, float("nan")) if q8 and kind == "inner" else lo16, "v": v}
    if q8:
        out["hi8"] = _e4m3(u.clamp(0.0, 448.0))
        out["lo8"] = _e4m3((lo16 if fault == "lo8_from_lo16" and kind == "out" else l) * 2.0 ** PR.LO_SHIFT)
        if fault == "inner_lo8_zero" and kind == "inner":
            out["lo8"] = torch.zeros_like(h)
    return out


def standin_stem_pool(mode: str, form: str, inp: torch.Tensor, W: dict) -> dict:
    if form == "u8_strip":
        st = W["stem_u8"]
        mu = 255.0 * torch.tensor(IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
        c = _f(F.pad(inp.permute(0, 3, 1, 2).to(torch.float64) - mu, (3, 3, 3, 3)))  # the reference pads with the normalised 0
        b0 = _f(W["stem"]["b"] * 2.0 ** st["S"]).view(1, -1, 1, 1)
        a = (F.conv2d(c, _f(st["whi"]), None, stride=2) + F.conv2d(c, _f(st["wlo"]), None, stride=2)) + b0
        v = F.max_pool2d(a.clamp_min(0), 3, 2, 1) * 2.0 ** -st["S"]
    else:
        a = F.conv2d(_f(inp), _f(W["stem"]["w"]), None, stride=2, padding=3) + _f(W["stem"]["b"]).view(1, -1, 1, 1)
        v = F.max_pool2d(a.clamp_min(0), 3, 2, 1)
    h = v.to(torch.float16).to(torch.float32)
    lo16 = (v - h).to(torch.float16).to(torch.float32)
    out = {"hi": h, "lo": lo16, "v": v}
    if mode == "fp16q8":  # from the stored halves, in both forms
        out["hi8"], out["lo8"] = _e4m3(h), _e4m3(lo16 * 2.0 ** PR.LO_SHIFT)
    return out


def standin_forward(mode: str, inp: torch.Tensor, W: dict, stem: str = "u8_strip", pool_head: bool = True, fault: Optional[str] = None) -> dict:
    """The stand-in run FREELY through the trunk (each conv fed by its own output) -> the ``dev`` dict of
    ``PR.check_forward`` (every plane a float32 tensor; ``PR`` converts)."""
    dev = {"input": inp, "pool": standin_stem_pool(mode, stem, inp, W), "inner": [], "out": []}
    X = dev["pool"]
    for i, name in enumerate(PR.BLOCKS):
        w, pl = W[name], PR.conv_plan(i)
        t = standin_conv(mode, X, w["conv1"], "inner", pl["stride"], fault=fault)
        kind = "last" if i == 7 else "out"
        if pl["proj"]:
            o = standin_conv(mode, t, w["conv2"], kind, proj_x=X, proj_w=w["proj"], S_own=w["S_proj_own"], fault=fault)
        else:
            o = standin_conv(mode, t, w["conv2"], kind, resid=X, fault=fault)
        dev["inner"].append(t)
        dev["out"].append(o)
        X = o
    dev["feats"], dev["logits"] = IC.emulate_head(X["f32"], W["fc"], pool_head)
    return dev


def to64(dev: dict) -> dict:
    """The planes as float64 tensors, as ``PR.decode_*`` deliver the device's."""
    def cv(v):
        if isinstance(v, dict):
            return {k: cv(t) for k, t in v.items()}
        if isinstance(v, list):
            return [cv(t) for t in v]
        return v.to(torch.float64) if v.is_floating_point() else v
    return {k: cv(v) for k, v in dev.items()}


def value_of(planes: dict) -> torch.Tensor:
    """What capi.PackedResNet18.tap returns for the map: (float)hi + (float)lo, or the fp32 map."""
    return planes["f32"] if "f32" in planes else planes["hi"] + planes["lo"]


def standin_distances(mode: str, dev: dict, W: dict, stem: str) -> Dict[str, tuple]:
    """(max|v - ref| / max|ref|, {slice kind: PR.slice_rms(v - ref) / max|ref|}) per conv stage (and "stem_pool_" + stem) of one stand-in forward ``dev`` (float64 planes, "v"
    included): the d of the oracle's tolerance, measured on the UNROUNDED float32 epilogue value against the float64 replay
    from the stand-in's own operand planes."""
    rel = lambda v, ref: (float((v - ref).abs().max() / ref.abs().max()), {k: r / float(ref.abs().max()) for k, r in PR.slice_rms(v - ref).items()})  # noqa: E731
    out = {"stem_pool_" + stem: rel(dev["pool"]["v"], PR.stem_pool_ref(stem, dev["input"], W))}
    X = dev["pool"]
    for i, name in enumerate(PR.BLOCKS):
        w, pl = W[name], PR.conv_plan(i)
        out[name + ".conv1"] = rel(dev["inner"][i]["v"], PR.conv_ref(mode, X, w["conv1"], pl["stride"]))
        kw = dict(proj_x=X, proj_w=w["proj"]) if pl["proj"] else dict(resid=X)
        out[name + ".conv2"] = rel(dev["out"][i]["v"], PR.conv_ref(mode, dev["inner"][i], w["conv2"], 1, **kw))
        X = dev["out"][i]
    return out
