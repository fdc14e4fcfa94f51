"""Cases shared by tests/test_oracle_infer_replay.py (CPU) and tests/test_gpu_infer_replay.py, and the CPU STAND-IN of the
device: an independent emulation of the inference trunk with torch FLOAT32 convolutions (a summation order that is neither
the device's nor the float64 replay's) and the device's rounding sites (oracle/infer_replay.py, module docstring).  The
strip stem is emulated WITHOUT the bias table -- b0 + the sum over the taps inside the image of rw (v - 255 mean_c) -- so
that the table's algebra is checked and not copied.

The stand-in can be built with ONE FAULT, the kind of error that fits inside the end-to-end tests' 3 %:
  block   "drop_tap_col0"     conv2's centre tap -- offset (0, 0); the tap of KERNEL INDEX (0, 0) reads only padding at output
                              column 0, so dropping it there changes nothing -- left out for output column 0 only
          "swap_channels"     two input channels of one 32-channel chunk exchanged in W2
          "unrounded_inner"   the inner map kept in float32
          "rtz_out"           the output rounded towards zero instead of to nearest even
          "no_proj_bias"      the projection's bias left out of the folded bias
  stem    "pad_m128_last_row" strip stem: the bias table's last ROW class does not take back the 128 w of the taps below the
                              image, i.e. the padding there reads as byte -128 instead of the normalised 0
  head    "half_wave"         split-sum head: image 2 of a batch (pixels 98 .. 146 of the flattened 7 x 7 maps) straddles
                              the 128-pixel wave half and loses the pixels beyond it
          "swap_3_4"          the features of images 3 and 4 exchanged
"""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

import rescale_cases
from oracle import infer_replay as IR
from oracle.transform_ref import IMAGENET_MEAN, IMAGENET_STD, to_tensor_normalize
from ss25_hierarchical_multiscale_image_classification_amd import synth

WEIGHT_SEED = 2
PRECISIONS = ("bf16", "fp16", "fp32")


def state_dict(kind: str = "plain") -> Dict[str, torch.Tensor]:
    """"plain": the seeded Kaiming weights; "rescaled": the same function with the inner magnitudes spread over 2^-4 .. 2^4."""
    sd = synth.seeded_resnet18_state_dict(WEIGHT_SEED, 2)
    return rescale_cases.rescale_inner(sd, 4, seed=WEIGHT_SEED + 100) if kind == "rescaled" else sd


def patches(n: int, seed: int = 21) -> torch.Tensor:
    """uint8 [n,224,224,3] random patches with extreme values along all four borders (tests/test_gpu_resnet.py:_border_patches)."""
    u8 = synth.synth_patches_u8(max(n, 3), seed=seed)
    u8[0, :5] = 0
    u8[1, :, -3:] = 255
    u8[2, -4:, :] = 255
    u8[2, :, :2] = 0
    if n < 3:  # the small batches keep every border: the last patch takes the third one's
        u8[n - 1, -4:, :] = 255
        u8[n - 1, :, :2] = 0
    return u8[:n].contiguous()


def normalized(u8: torch.Tensor) -> torch.Tensor:
    """float32 [n,3,224,224]: ToTensor + Normalize as torchvision does them."""
    return torch.stack([torch.from_numpy(to_tensor_normalize(p.numpy())) for p in u8])


def normalized64(u8: torch.Tensor) -> torch.Tensor:
    """float64 [n,3,224,224]: the same transform evaluated in float64."""
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1)
    return (u8.permute(0, 3, 1, 2).to(torch.float64) / 255.0 - mean) / std


# ---------------------------------------------------------------------------------------------------------------------
# the float32 stand-in
# ---------------------------------------------------------------------------------------------------------------------
def _r(t: torch.Tensor, storage) -> torch.Tensor:
    return t if storage in (None, torch.float32) else t.to(storage).to(torch.float32)


def _rtz(t: torch.Tensor, storage) -> torch.Tensor:
    if storage == torch.float32:
        return t
    h = t.to(storage)
    over = h.to(torch.float32).abs() > t.abs()  # rounded away from zero: one step back (sign-magnitude bits)
    return torch.where(over, (h.view(torch.int16) - 1).view(storage), h).to(torch.float32)


def _w(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32)


def _conv(x, w, stride=1):
    return F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2)


def emulate_stem(form: str, inp: torch.Tensor, Fd: dict, storage, fault: Optional[str] = None):
    """-> (stem map, pooled map), float32 tensors of T values."""
    b = _w(Fd["stem"]["b"]).view(1, -1, 1, 1)
    if form == "u8_strip":
        mu = 255.0 * torch.tensor(IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
        c = F.pad(inp.permute(0, 3, 1, 2).to(torch.float64) - mu, (3, 3, 3, 3))  # the reference pads with the normalised 0
        if fault == "pad_m128_last_row":
            c[:, :, 227:, :] = -128.0
        a = F.conv2d(c.to(torch.float32), _w(Fd["stem_u8"]["rw"]), None, stride=2) + b
    else:
        if form == "u8_table":
            lut = IR.normalize_lut(storage).to(torch.float32)
            v = inp.permute(0, 3, 1, 2).long()
            x = torch.stack([lut[ch][v[:, ch]] for ch in range(3)], dim=1)
        else:
            x = _r(inp.to(torch.float32), storage)
        a = _conv(x, _w(Fd["stem"]["w"]), 2) + b
    stem = _r(a.clamp_min(0), storage)
    return stem, F.max_pool2d(stem, 3, 2, 1)


def emulate_block(X: torch.Tensor, w: dict, kind: str, storage, last: bool = False, fault: Optional[str] = None) -> torch.Tensor:
    X = X.to(torch.float32)
    stride = 1 if kind == "identity" else 2
    t = (_conv(X, _w(w["w1"]), stride) + _w(w["b1"]).view(1, -1, 1, 1)).clamp_min(0)
    if fault != "unrounded_inner":
        t = _r(t, storage)
    W2 = _w(w["w2"])
    if fault == "swap_channels":
        W2 = W2.clone()
        W2[:, [35, 49]] = W2[:, [49, 35]]  # both in the chunk of channels 32 .. 63
    o = _conv(t, W2)
    if fault == "drop_tap_col0":
        o[..., 0] -= F.conv2d(t, W2[:, :, 1:2, 1:2])[..., 0]
    if kind == "identity":
        o = o + _w(w["b2"]).view(1, -1, 1, 1) + X
    elif kind == "projk":
        bias = w["b2"] if fault == "no_proj_bias" else w["bias_c2p"]
        o = o + _conv(X, _w(w["wp"]), 2) + _w(bias).view(1, -1, 1, 1)
    else:
        p = _conv(X, _w(w["wp"]), 2)
        if fault != "no_proj_bias":
            p = p + _w(w["bp"]).view(1, -1, 1, 1)
        o = o + _w(w["b2"]).view(1, -1, 1, 1) + _r(p, storage)
    o = o.clamp_min(0)
    if last:
        return o
    return _rtz(o, storage) if fault == "rtz_out" else _r(o, storage)


def emulate_head(last: torch.Tensor, fc: dict, pool_head: bool, fault: Optional[str] = None):
    """-> (features, logits) of the float32 last map [B,512,7,7]."""
    v = last.to(torch.float32)
    if pool_head:  # halo16.h POOL: hi on the grid 2^-10, lo on the grid 2^-29, both sums exact; the rest is dropped
        hi = (v + 12288.0) - 12288.0
        lo = ((v - hi) + 0.0234375) - 0.0234375
        keep = torch.ones(v.shape[0], 1, 49, dtype=torch.float64)
        if fault == "half_wave":
            keep[2, 0, 128 - 2 * 49:] = 0.0
        s = lambda t: (t.flatten(2).to(torch.float64) * keep).sum(dim=2).to(torch.float32)  # noqa: E731
        feats = (s(hi) + s(lo)) / 49.0
    else:
        acc = torch.zeros(v.shape[:2], dtype=torch.float32)
        for p in range(49):
            acc = acc + v.flatten(2)[:, :, p]
        feats = acc / 49.0
    if fault == "swap_3_4":
        feats = feats.clone()
        feats[[3, 4]] = feats[[4, 3]]
    return feats, feats @ _w(fc["w"]).t() + _w(fc["b"])


def emulate(inp: torch.Tensor, Fd: dict, storage, stem: str = "u8_strip", fuse_stem: bool = True, projk: bool = True,
            pool_head: bool = True) -> dict:
    """The whole stand-in forward -> the ``dev`` dict of ``infer_replay.check_forward``."""
    if storage == torch.float32:
        fuse_stem = projk = pool_head = False
    stem_map, pool = emulate_stem(stem, inp, Fd, storage)
    dev = {"input": inp, "pool": pool, "blocks": []}
    if not fuse_stem:
        dev["stem"] = stem_map
    X = pool
    for i, name in enumerate(IR.BLOCKS):
        X = emulate_block(X, Fd[name], IR.block_kind(name, storage, projk), storage, last=i == 7)
        dev["blocks"].append(X)
    dev["feats"], dev["logits"] = emulate_head(X, Fd["fc"], pool_head)
    return dev
