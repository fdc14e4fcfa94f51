"""A function-preserving rescaling of ResNet18 state dicts, shared by tests/test_rescale_host.py,
tests/test_gpu_resnet_rescaled.py and tests/tools/prec_mx.py.

Inside a BasicBlock  conv1 -> bn1 -> ReLU -> conv2  the ReLU is positively homogeneous, so scaling channel c of bn1's affine
(weight and bias) by a_c > 0 and conv2's input channel c by 1 / a_c leaves the block's function unchanged.  With a_c a power
of two every product involved is exact in fp32: the fp32 oracle's outputs are bit-identical.  What moves is the block's inner
activation and the two convs' folded weights -- by up to 2^K either way, per channel -- which is what a trained checkpoint
looks like and what the seeded Kaiming state dicts (all weights and activations within a factor ~4) do not.  Stem, max-pool and
the eight block outputs (every tap of the C ABI) keep their values.
"""
from typing import Dict

import torch

BLOCKS = tuple(f"layer{s}.{b}" for s in (1, 2, 3, 4) for b in (0, 1))


def rescale_inner(sd: Dict[str, torch.Tensor], K: int, seed: int) -> Dict[str, torch.Tensor]:
    """A copy of the (bare torchvision-named) state dict `sd` with, per BasicBlock and per channel c of its bn1, bn1's weight
    and bias times 2^k_c and conv2.weight[:, c] times 2^-k_c; k_c integer, uniform in [-K, K], drawn block by block from
    torch.Generator().manual_seed(seed).  K = 0 returns an equal copy."""
    gen = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    for p in BLOCKS:
        n = out[p + ".bn1.weight"].shape[0]
        k = torch.randint(-K, K + 1, (n,), generator=gen)
        a = torch.exp2(k.to(torch.float32))
        out[p + ".bn1.weight"] = out[p + ".bn1.weight"] * a
        out[p + ".bn1.bias"] = out[p + ".bn1.bias"] * a
        out[p + ".conv2.weight"] = out[p + ".conv2.weight"] / a[None, :, None, None]
    return out


def folded(sd: Dict[str, torch.Tensor], conv: str, bn: str, eps: float = 1e-5):
    """(weight, bias) of conv + inference BN folded in double, as the library's packer folds them."""
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + eps)
    return sd[conv + ".weight"].double() * s[:, None, None, None], sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s


def conv_bn_pairs(sd: Dict[str, torch.Tensor]):
    """Every (conv, bn) name pair of the network, stem and projections included."""
    pairs = [("conv1", "bn1")]
    for p in BLOCKS:
        pairs += [(p + ".conv1", p + ".bn1"), (p + ".conv2", p + ".bn2")]
        if (p + ".downsample.0.weight") in sd:
            pairs.append((p + ".downsample.0", p + ".downsample.1"))
    return pairs
