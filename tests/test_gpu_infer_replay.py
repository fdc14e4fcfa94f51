"""The inference trunk that is shipped and timed (bf16 / fp16: stem.h, block16_c64.h, halo16.h, conv_glds.h, the pooled head;
fp32: conv_f32.hip) BLOCK BY BLOCK against oracle/infer_replay.py, through capi.PackedResNet18: ``forward``, then ``tap``.

tests/test_gpu_resnet*.py and test_gpu_pipeline.py compare these modes with the fp32 oracle end to end at 2.5e-2 / 3e-2 (bf16)
and 1e-3 - 3e-3 (fp16) of a map's largest value: a filter tap missing along one border, two channels swapped in a packed chunk,
a ragged tile read from the neighbouring image, a pooled-epilogue slot that loses pixels or a projection folded with the wrong
bias all fit inside.  Here every stage is recomputed in float64 FROM THE DEVICE'S OWN INPUT MAP with the device's quantised
weights, so that one rounding lies between the given input and the checked output; the bounds are derived per element and no
element is left out (oracle/infer_replay.py: the rounding sites, the interval of the block check, the mean-square statistic).

All patches go to the device; the listed images are replayed on the CPU one at a time.
  precision    input      knobs                      batch: replayed    what it reaches
  bf16, fp16   uint8      default                    7: all             strip stem; fused layer1; folded projections; pooled head with
                                                                        images crossing a wave half (image 2) and a 256-pixel tile (5)
  bf16         uint8      default                    1: 0               idle workgroups; lone-tile paths
  bf16, fp16   uint8      default, rescaled weights  3: all             magnitude spread
  bf16         uint8      default                    70: 0, 5, 37, 69   workgroups that walk several strips and tiles; ragged last tiles
                                                                        at 14 x 14 and 7 x 7
  bf16, fp16   nchw_f32   default                    2: all             tile stem kernel on NHWC4 input
  bf16         uint8      HIPAC_STEM_STRIP=0         2: all             byte table through the tile kernel
  bf16, fp16   nchw_f32   HIPAC_FUSE_STEM=0          2: all             stem tap and pool tap checked separately
  bf16         uint8      HIPAC_L1_FUSED=0 /         3: all             separate convs; rounded projection maps (launch_down in layers
                          HIPAC_PROJK=0 /                               2-3, its own launch in layer 4); head_kernel
                          HIPAC_POOL_HEAD=0
  fp32         nchw_f32   default                    2: all             conv_f32.hip, u = 2^-24
Asserted: every stage's ratio <= 1 (no element outside its interval), every block's mean-square statistic below its gate, and
labels == argmax(device logits).  fp16x3 and fp16q8 are replayed conv by conv in
tests/test_gpu_pair_replay.py (the oracle's docstring says why they need another method).

Every figure is printed by the test (ratio / fig / sqrtK / msq per stage).  Measured on an MI355X, worst case of each
precision, with the float32 stand-in of tests/infer_replay_cases.py on the same cases in brackets:
          stem ratio      stem sqrtK      block fig        block sqrtK    block msq        feats ratio      feats sqrtK    logits ratio
  bf16    0.990 [0.990]   0.028 [0.088]   1.03 [1.10]      6.7 [6.7] (*)  0.914 [0.915]    0.557 [0.536]    0.24 [0.23]    3.2e-4 [1.6e-3]
  fp16    0.946 [0.946]   0.046 [0.191]   0.852 [0.850]    4.2 [4.2]      0.750 [0.752]    0.544 [0.539]    0.23 [0.23]    4.4e-4 [6.7e-4]
  fp32    0.038 [0.038]   0.444 [0.444]   2.7e-4 [2.7e-4]  0.09 [0.06]    0.000 [0.000]    0.123 [0.105]    0.88 [0.75]    3.0e-4 [5.3e-4]
(*) 37 [9.4] with HIPAC_PROJK=0: one element of a projection map sits a unit of bf16 from its float64 rounding, which the
interval allows and the unit counts as a rare event.  head_kernel (HIPAC_POOL_HEAD=0, bf16): features 0.117 [0.104], sqrtK
0.84 [0.74].  No element of any stage lay outside its interval; the device's figures are the stand-in's almost digit for digit,
i.e. what is left of the bounds is the reference arithmetic's own rounding, not the kernels'.
"""
import pytest
import torch

import infer_replay_cases as cases
from oracle import infer_replay as IR
from ss25_hierarchical_multiscale_image_classification_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def folded():
    cache = {}

    def get(kind, prec):
        if (kind, prec) not in cache:
            cache[(kind, prec)] = (cases.state_dict(kind), IR.fold(cases.state_dict(kind), IR.STORAGE[prec]))
        return cache[(kind, prec)]
    return get


def _check(folded, prec, n, images, weights="plain", inp="u8", stem=None, fuse=True, projk=True, pool_head=True):
    """One forward of ``n`` patches on the device (the knobs are already in the environment), its taps, and the replay of ``images``."""
    sd, Fd = folded(weights, prec)
    st = IR.STORAGE[prec]
    if prec == "fp32":
        fuse = projk = pool_head = False
    u8 = cases.patches(n)
    x = cases.normalized(u8) if inp == "nchw_f32" else u8
    form = stem or ("nchw_f32" if inp == "nchw_f32" else "u8_strip")
    net = capi.PackedResNet18(sd, precision=prec)
    feats, logits, labels = net.forward(x.cuda(), want_logits=True, want_labels=True)
    assert torch.equal(labels, logits.argmax(1))
    idx = torch.tensor(list(images)).cuda()
    tap = lambda t: net.tap(n, t)[idx].cpu()  # noqa: E731
    dev = {"input": x[list(images)], "pool": tap(1), "blocks": [tap(2 + i) for i in range(8)], "feats": feats[idx].cpu(), "logits": logits[idx].cpu()}
    if not fuse:
        dev["stem"] = tap(0)
    else:
        with pytest.raises(capi.HipacError):
            net.tap(n, 0)  # the fused forms never materialise the stem map
    res = IR.check_images(dev, range(len(images)), Fd, st, stem=form, projk=projk, pool_head=pool_head)
    for r in res.values():  # name the image by its place in the batch
        r["worst"] = (images[r["worst"][0]],) + tuple(r["worst"][1:]) if r["worst"] else r["worst"]
    tag = f"{prec} {weights} {form} n={n} images={list(images)} fuse={fuse} projk={projk} pool_head={pool_head}"
    print(f"{tag}\n{IR.summary(res)}")
    kinds = {"stem": [s for s in res if s.startswith("stem")], "block": list(IR.BLOCKS), "feats": ["feats"], "logits": ["logits"]}
    print(f"{tag}: " + "; ".join(f"{k} ratio {max(res[s]['ratio'] for s in v):.3f} fig {max(res[s]['fig'] for s in v):.3g} "
                                 f"sqrtK {max(res[s]['sqrtk'] for s in v):.3g}" for k, v in kinds.items())
          + f"; block msq {max(res[s]['msq'] for s in IR.BLOCKS):.3f}")
    assert set(res) == ({"stem_pool"} if fuse else {"stem", "pool"}) | set(IR.BLOCKS) | {"feats", "logits"}
    assert not IR.failures(res), (tag, IR.failures(res))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_default_uint8_path_seven_patches(folded, prec):
    """7 x 49 pixels of the last map: image 2 (pixels 98 .. 146) crosses the 128-pixel wave half, image 5 (245 .. 293) the tile."""
    _check(folded, prec, 7, range(7))


def test_default_uint8_path_one_patch(folded):
    _check(folded, "bf16", 1, [0])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_default_uint8_path_rescaled_weights(folded, prec):
    _check(folded, prec, 3, range(3), weights="rescaled")


def test_default_uint8_path_seventy_patches(folded):
    """70 patches: workgroups walk several strips and tiles, and the last 256-pixel tiles of layers 3 and 4 are ragged
    (70 x 196 = 53 x 256 + 152, 70 x 49 = 13 x 256 + 102).  Four images are replayed: the first, the last, and two inside."""
    _check(folded, "bf16", 70, [0, 5, 37, 69])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_float_input_tile_stem(folded, prec):
    _check(folded, prec, 2, range(2), inp="nchw_f32")


def test_uint8_table_through_the_tile_stem(folded, monkeypatch):
    monkeypatch.setenv("HIPAC_STEM_STRIP", "0")
    _check(folded, "bf16", 2, range(2), stem="u8_table")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_unfused_stem_and_pool(folded, monkeypatch, prec):
    monkeypatch.setenv("HIPAC_FUSE_STEM", "0")
    _check(folded, prec, 2, range(2), inp="nchw_f32", fuse=False)


@pytest.mark.parametrize("knob", ["HIPAC_L1_FUSED", "HIPAC_PROJK", "HIPAC_POOL_HEAD"])
def test_one_knob_off(folded, monkeypatch, knob):
    monkeypatch.setenv(knob, "0")  # before the handle is made: HIPAC_PROJK is read at pack time
    _check(folded, "bf16", 3, range(3), projk=knob != "HIPAC_PROJK", pool_head=knob != "HIPAC_POOL_HEAD")


def test_fp32_mode(folded):
    _check(folded, "fp32", 2, range(2), inp="nchw_f32")
