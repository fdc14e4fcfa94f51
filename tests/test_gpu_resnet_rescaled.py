"""The HIP ResNet18 forward on state dicts whose inner channels are spread over powers of two (rescale_cases.rescale_inner:
per BasicBlock, bn1's affine of channel c times 2^k_c, conv2's input channel c times 2^-k_c, k_c in [-K, K]).  The transform
leaves the network's function and the fp32 oracle's bits unchanged (tests/test_rescale_host.py), so the oracle run on the seeded
state dict is the reference for its rescaled forms too; what changes is the magnitude of the folded weights and of each block's
inner activation -- which the seeded Kaiming weights of every other test keep within a factor ~4 and a trained checkpoint does not.

Bounds: TOL of tests/test_gpu_resnet.py, imported, unchanged.  Norm-relative errors (max|a-b| / max|b|) against the oracle on 4
patches, uint8 input, measured on MI355X in brackets [seed 0 / seed 2]; "before" = the pair weights packed unscaled (the parent
commit's library on the same inputs), "now" = pack_conv_pairs scaling every conv's weights by its own 2^S:
                    features                 logits                   worst tap
    fp16x3  K = 0   before [1.6e-6 / 1.2e-6] [2.8e-6 / 9.0e-7] [2.6e-6 / 2.3e-6]   now [3.9e-7 / 4.5e-7] [1.7e-6 / 6.7e-7] [1.5e-6 / 1.9e-6]
    fp16x3  K = 4   before [7.6e-6 / 6.5e-6] [1.4e-5 / 7.6e-6] [1.3e-5 / 9.8e-6]   now [3.9e-7 / 3.9e-7] [2.0e-6 / 9.0e-7] [2.0e-6 / 1.5e-6]   bound 2e-5
    fp16x3  K = 8   before [8.4e-5 / 8.9e-5] [7.3e-4 / 9.9e-5] [1.4e-4 / 1.1e-4]   now [7.5e-7 / 6.1e-7] [4.5e-6 / 9.0e-7] [3.4e-6 / 2.3e-6]   bound 2e-5
    fp16q8  K = 0   before [1.1e-5 / 9.8e-6] [3.6e-5 / 1.6e-5] [4.2e-5 / 3.4e-5]   now [7.9e-6 / 1.3e-5] [4.3e-5 / 1.8e-5] [3.7e-5 / 3.3e-5]
    fp16q8  K = 4   before [1.7e-5 / 1.2e-5] [5.4e-5 / 1.7e-5] [4.4e-5 / 3.8e-5]   now [8.2e-6 / 1.2e-5] [3.9e-5 / 1.4e-5] [3.5e-5 / 3.3e-5]   bound 1e-4
    fp16q8  K = 8   before [8.2e-5 / 8.7e-5] [7.5e-4 / 8.6e-5] [1.6e-4 / 1.4e-4]   now [1.3e-4 / 7.9e-5] [5.0e-4 / 9.5e-5] [2.2e-4 / 2.0e-4]   not asserted
    fp32    K = 4, 8 (the same bits)         [4.6e-7 / 4.5e-7] [2.5e-6 / 7.8e-7] [1.7e-6 / 1.9e-6]                                  bound 2e-5
    fp16    K = 4                            [5.3e-4 / 5.0e-4] [1.0e-3 / 4.5e-4] [1.1e-3 / 1.0e-3]                                  bounds 1e-3 / 2e-3 / 3e-3
(float input, now: fp16x3 K = 4 logits [1.3e-6 / 9.0e-7], K = 8 [4.3e-6 / 9.0e-7]; fp16q8 K = 4 [3.8e-5 / 1.3e-5].)
Unscaled, both pair modes lose precision with the spread: fp16x3 breaks its bound at K = 8 by a factor 36 and is no better there than
one fp16 product; at K = 4 the device stayed inside the bounds (the CPU emulation on 2 patches had put it just outside).  With the
per-conv scale fp16x3 does not notice the spread.  fp16q8 is unchanged at K <= 4, and at K = 8 its error is the activation side's.
fp16q8 at K = 8 is NOT asserted.  The e4m3 window of the ACTIVATIONS' byte planes is fixed by design (hi8 = e4m3(xhi) saturates at
448 and loses mantissa below 2^-6; an inner activation spread over 2^+-8 leaves it), the per-conv weight scale cannot help there, and
the CPU emulation (tests/tools/prec_mx.py 2 --rescale 8) leaves the logits at 5.6e-4.  It is measured (above) and stays
inside north_star's 1e-3 there, no more.

Scale invariance: for bf16 and fp32 the device must give the SAME BITS for a state dict and its K = 4 rescaled form -- rounding to
bf16, exact-f32 / bf16 MFMA products and fp32 accumulation all commute with a power-of-two factor when the summation order is the
same -- so the test needs no tolerance and fails on any hidden dependence on magnitude.  The single-product fp16 mode gets no bit
claim (folded weights below 2^-14 are fp16 subnormals), only its existing TOL against the oracle.
"""
import functools

import pytest
import torch

import rescale_cases
from oracle import resnet18_ref as R, transform_ref as T
from ss25_hierarchical_multiscale_image_classification_amd import capi, synth
from test_gpu_resnet import TAPS, TOL, WIDE, rel

pytestmark = pytest.mark.gpu
N = 4


@functools.lru_cache(maxsize=None)
def patches():
    u8 = synth.synth_patches_u8(N, seed=1)
    return u8, torch.stack([torch.from_numpy(T.to_tensor_normalize(p.numpy())) for p in u8])


@functools.lru_cache(maxsize=None)
def oracle(seed):
    """(state dict, features, logits, taps) of the fp32 oracle: computed once per seed, shared, never written to."""
    sd = synth.seeded_resnet18_state_dict(seed, num_classes=2)
    taps = {}
    f, l = R.resnet18_forward(patches()[1], sd, taps)
    return sd, f, l, taps


def rescaled(seed, K):
    sd = oracle(seed)[0]
    return rescale_cases.rescale_inner(sd, K, seed=100 + seed) if K else sd


def run_device(prec, sd, path):
    """One pack, one forward of the 4 patches -> (features, logits, labels, {tap index: map}) on the host."""
    u8, x = patches()
    net = capi.PackedResNet18(sd, precision=prec)
    f, l, lab = net.forward(u8.cuda() if path == "u8" else x.cuda(), want_feats=True, want_logits=True, want_labels=True)
    # the stem map (tap 0) is materialised by fp32 on either input, by the pair modes on float input only (their uint8 strip kernel
    # pools in registers), by bf16 / fp16 never (fused stem)
    has_stem = prec == "fp32" or (prec in WIDE and path == "nchw_f32")
    taps = {i: net.tap(N, i).cpu() for i in range(len(TAPS)) if i > 0 or has_stem}
    return f.cpu(), l.cpu(), lab.cpu(), taps


def errors(prec, seed, K, path="u8"):
    """Device against oracle: (features, logits, worst tap and its name, labels, logits)."""
    _, ref_f, ref_l, ref_taps = oracle(seed)
    f, l, lab, taps = run_device(prec, rescaled(seed, K), path)
    tap_err = {TAPS[i]: rel(t, ref_taps[TAPS[i]]) for i, t in taps.items()}
    worst = max(tap_err, key=tap_err.get)
    return rel(f, ref_f), rel(l, ref_l), tap_err[worst], worst, lab, l


def check_against_oracle(prec, seed, K, path):
    _, _, ref_l, _ = oracle(seed)
    ef, el, et, worst, lab, l = errors(prec, seed, K, path)
    print(f"rescaled {prec} seed {seed} K {K} {path}: features {ef:.2e} logits {el:.2e} worst tap {et:.2e} ({worst})")
    assert ef <= TOL[prec]["feat"]
    assert el <= TOL[prec]["out"]
    assert et <= TOL[prec]["tap"], worst
    margin = (ref_l[:, 0] - ref_l[:, 1]).abs()
    decided = margin > 2 * TOL[prec]["out"] * float(ref_l.abs().max())
    assert torch.equal(lab[decided], ref_l.argmax(1)[decided])
    assert torch.equal(lab, l.argmax(1))


PARITY_CASES = [(prec, 4, "u8") for prec in ("fp16x3", "fp16q8", "fp32")] + [(prec, 8, "u8") for prec in ("fp16x3", "fp32")] + \
               [("fp16x3", 4, "nchw_f32"), ("fp16q8", 4, "nchw_f32"), ("fp16x3", 8, "nchw_f32")]


@pytest.mark.parametrize("seed", [0, 2])
@pytest.mark.parametrize("prec,K,path", PARITY_CASES)
def test_parity_under_rescale(prec, K, path, seed):
    check_against_oracle(prec, seed, K, path)


@pytest.mark.parametrize("seed", [0, 2])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_scale_invariance_bit_for_bit(prec, seed):
    f0, l0, lab0, taps0 = run_device(prec, rescaled(seed, 0), "u8")
    f1, l1, lab1, taps1 = run_device(prec, rescaled(seed, 4), "u8")
    assert sorted(taps0) == sorted(taps1) == list(range(0 if prec == "fp32" else 1, len(TAPS)))
    for i in taps0:
        assert torch.equal(taps0[i], taps1[i]), TAPS[i]
    assert torch.equal(f0, f1) and torch.equal(l0, l1) and torch.equal(lab0, lab1)


@pytest.mark.parametrize("seed", [0, 2])
def test_single_product_fp16_under_rescale(seed):
    check_against_oracle("fp16", seed, 4, "u8")
