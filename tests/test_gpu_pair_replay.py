"""The pair modes of the inference trunk (fp16x3, fp16q8: halo16x2.h, the SPLIT / Q8 strip stem, pool.h's split pool,
pairs_to_q8_kernel) CONV BY CONV against oracle/pair_replay.py, through capi.PackedResNet18: ``forward``, then ``raw_tap`` (the
stored pair and byte tensors, copied byte for byte; a block's inner map after ``run_ops`` of its first conv alone).

tests/test_gpu_resnet*.py hold these modes to 2e-5 / 1e-4 of a map's largest value end to end; a tap dropped along one border,
two channels exchanged in a packed chunk or a byte plane made from the wrong operand pass the 1e-4 of fp16q8, the benchmark's
parity mode (tests/test_oracle_pair_replay.py has the figures).  Here every conv is recomputed in float64 from the operand
planes the device stored, with the weights restated from the state dict, and compared per element against a gate of 10 x the
distance a float32 stand-in leaves (tests/golden/pair_replay_distances.json, measured on the CPU); no element is left out.

All patches go to the device; the listed images are replayed on the CPU one at a time.
  modes            input      knobs / weights      batch: replayed    what it reaches
  fp16x3, fp16q8   uint8      default              7: 0, 2, 5, 6      BN = 64 layer1 form with both residual planes in one round trip; BN = 128
                                                                      forms; layer4's 343 pixels = one full 256-pixel tile + 87 ragged; pooled
                                                                      slots crossing a wave half (image 2) and a tile (image 5); folded
                                                                      projections; stride-2 entry convs
  fp16q8           uint8      default              1: 0               lone ragged tile (49 pixels), idle workgroups
  fp16x3, fp16q8   uint8      rescaled weights     3: all             a different S per conv; every folded projection's own S differs from
                                                                      its conv's (tests/test_oracle_pair_replay.py)
  fp16q8           uint8      default              70: 0, 5, 37, 69   workgroups walking several tiles; ragged last tiles at 14 x 14 and 7 x 7
  fp16x3, fp16q8   nchw_f32   HIPAC_STEM_STRIP=0   2: all             exact f32 stem, split pool, pairs_to_q8_kernel
  fp16q8           uint8      HIPAC_POOL_HEAD=0    3: all             OUTF32 last conv + head_kernel
Asserted: every stage's ratio <= 1 (every check of the oracle's docstring, every element), labels == argmax(device logits), and
the raw pooled and block-output planes, summed, equal ``tap`` bit for bit for every image of the batch (the new tap is tied to
the old one).  Every figure is printed by the test.

Measured on an MI355X, the worst case of each mode over the cases above: the plain distance max|dev - ref| / max|ref| per stage
kind, with the float32 stand-in's figure (the d of the gate; the gate is 10 x that) in brackets, the worst ratio of the head's
checks (oracle/infer_replay.py), and the lowest tie rate m / T of any replayed image and map with T >= 100:
          stem + pool        conv1 (inner map)       conv2 (pairs)       last map (fp32)     feats   logits    tie rate
  fp16x3  4.8e-7 [5.8e-7]    1.9e-6 [2.1e-6]         1.2e-6 [8.2e-7]     1.1e-6 [1.2e-6]     0.557   4.4e-4
  fp16q8  4.8e-7 [5.8e-7]    1.5e-5 (*) [2.1e-6]     1.0e-6 [9.2e-7]     1.1e-6 [1.2e-6]     0.572   4.7e-4    0.148 [0.151]
(*) an fp16q8 inner map has no lo plane: its value is taken as hi + lo8 2^-11, and 1.5e-5 is e4m3's rounding of lo (2^-16 of the
value).  Its hi, hi8 and lo8 are checked by their intervals, not by this figure.
Worst ratio of the root-mean-square check per slice kind, both modes (1 is the gate, 0.1 the stand-in itself): channels 0.125,
rows 0.119, columns 0.114; of the sum check 0.15.
No element of any stage lay outside its interval.  The device's distances are the stand-in's, i.e. the order of an fp32 sum and
nothing else.
"""
import json
import os

import pytest
import torch

import pair_replay_cases as cases
from oracle import pair_replay as PR
from ss25_hierarchical_multiscale_image_classification_amd import capi

pytestmark = pytest.mark.gpu
DIST = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_replay_distances.json")))
CONV1_OP = (2, 4, 6, 9, 11, 14, 16, 19)  # trunk.h: the op of block b's first conv (stage 0 has four ops, the others five)
KINDS = {"stem_pool": ["stem_pool"], "conv1": [b + ".conv1" for b in PR.BLOCKS], "conv2": [b + ".conv2" for b in PR.BLOCKS[:7]],
         "last": ["layer4.1.conv2"]}


@pytest.fixture(scope="module")
def packed():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = (cases.state_dict(kind), PR.pack(cases.state_dict(kind)))
        return cache[kind]
    return get


def _fetch(net, xg, n, images, mode):
    """The planes of ``images`` of the forward that just ran; every raw output plane of the whole batch against ``tap`` first."""
    q8 = mode == "fp16q8"
    idx = torch.tensor(list(images)).cuda()

    def planes(m, raw):
        if m == capi.PAIR_TAP_BLOCK0 + 7:
            return PR.decode_f32(raw[idx].cpu())
        p = PR.decode_pairs(raw[idx].cpu())
        if q8:
            p.update(PR.decode_q8(net.raw_tap(n, m, capi.PAIR_TAP_PLANE_Q8)[idx].cpu()))
        return p

    maps = []
    for m in range(capi.PAIR_TAP_POOL, capi.PAIR_TAP_BLOCK0 + 8):  # before any conv is re-run: map 9 re-runs the last one itself
        raw = net.raw_tap(n, m)
        if m == capi.PAIR_TAP_BLOCK0 + 7:
            summed = raw.view(torch.float32)
        else:
            h = raw.view(torch.float16)
            summed = h[..., :h.shape[-1] // 2].float() + h[..., h.shape[-1] // 2:].float()
        assert torch.equal(summed.permute(0, 3, 1, 2), net.tap(n, m)), f"raw map {m} and tap {m} differ"
        maps.append(planes(m, raw))
    inner = []
    for b in range(8):
        net.run_ops(xg, CONV1_OP[b], CONV1_OP[b])
        inner.append(planes(capi.PAIR_TAP_INNER0 + b, net.raw_tap(n, capi.PAIR_TAP_INNER0 + b)))
    return maps[0], inner, maps[1:]


def _check(packed, mode, n, images, weights="plain", inp="u8", pool_head=True):
    """One forward of ``n`` patches on the device (the knobs are already in the environment), its raw planes, and the replay of
    ``images``."""
    sd, W = packed(weights)
    u8 = cases.patches(n)
    x = cases.normalized(u8) if inp == "nchw_f32" else u8
    stem = "nchw_f32" if inp == "nchw_f32" else "u8_strip"
    net = capi.PackedResNet18(sd, precision=mode)
    xg = x.cuda()
    feats, logits, labels = net.forward(xg, want_logits=True, want_labels=True)
    assert torch.equal(labels, logits.argmax(1))
    pool, inner, out = _fetch(net, xg, n, images, mode)
    idx = torch.tensor(list(images)).cuda()
    dev = {"input": x[list(images)], "pool": pool, "inner": inner, "out": out, "feats": feats[idx].cpu(), "logits": logits[idx].cpu()}
    f2, l2, _ = net.forward(xg, want_logits=True)  # the fetch disturbed nothing a later forward depends on
    assert torch.equal(f2, feats) and torch.equal(l2, logits)
    res = PR.check_images(mode, dev, range(len(images)), W, DIST[mode], stem=stem, pool_head=pool_head)
    for r in res.values():  # name the image by its place in the batch
        r["worst"] = (images[r["worst"][0]],) + tuple(r["worst"][1:]) if r["worst"] else r["worst"]
    tag = f"{mode} {weights} {stem} n={n} images={list(images)} pool_head={pool_head}"
    print(f"{tag}\n{PR.summary(res)}")
    key = "stem_pool_" + stem
    stand = {"stem_pool": DIST[mode]["max"][key], **{k: max(DIST[mode]["max"][s] for s in v) for k, v in KINDS.items() if k != "stem_pool"}}
    print(f"{tag}: " + "; ".join(f"{k} dist {max(res[s]['dist'] for s in v):.3g} [stand-in {stand[k]:.3g}, gate {PR.FACTOR * stand[k]:.3g}] "
                                 f"rms ratio {max(max(res[s]['checks'].get('rms_' + q, 0.0) for q in PR.RMS_KINDS) for s in v):.3g}" for k, v in KINDS.items())
          + f"; feats ratio {res['feats']['ratio']:.3g}; logits ratio {res['logits']['ratio']:.3g}"
          + (f"; tie rate {min(r['tie']['m'] / max(r['tie']['T'], 1) for r in res.values() if 'tie' in r):.3g}" if mode == "fp16q8" else ""))
    assert set(res) == {"stem_pool"} | set(PR.CONVS) | {"feats", "logits"}
    assert not PR.failures(res), (tag, PR.failures(res))


@pytest.mark.parametrize("mode", PR.MODES)
def test_default_uint8_path_seven_patches(packed, mode):
    """7 x 49 pixels of the last map: image 2 (pixels 98 .. 146) crosses the 128-pixel wave half, image 5 (245 .. 293) the tile.
    Replayed: those two, the first and the last."""
    _check(packed, mode, 7, [0, 2, 5, 6])


def test_default_uint8_path_one_patch(packed):
    _check(packed, "fp16q8", 1, [0])


@pytest.mark.parametrize("mode", PR.MODES)
def test_default_uint8_path_rescaled_weights(packed, mode):
    _check(packed, mode, 3, range(3), weights="rescaled")


def test_default_uint8_path_seventy_patches(packed):
    """70 patches: workgroups walk several tiles, and the last 256-pixel tiles of layers 3 and 4 are ragged
    (70 x 196 = 53 x 256 + 152, 70 x 49 = 13 x 256 + 102).  Four images are replayed: the first, the last, and two inside."""
    _check(packed, "fp16q8", 70, [0, 5, 37, 69])


@pytest.mark.parametrize("mode", PR.MODES)
def test_float_input_unfused_stem(packed, monkeypatch, mode):
    monkeypatch.setenv("HIPAC_STEM_STRIP", "0")
    _check(packed, mode, 2, range(2), inp="nchw_f32")


def test_head_kernel_on_the_fp32_map(packed, monkeypatch):
    monkeypatch.setenv("HIPAC_POOL_HEAD", "0")
    _check(packed, "fp16q8", 3, range(3), pool_head=False)


def test_raw_tap_refuses_what_it_cannot_copy(packed):
    sd, _ = packed("plain")
    u8 = cases.patches(1).cuda()
    net = capi.PackedResNet18(sd, precision="fp16x3")
    with pytest.raises(capi.HipacError):
        net.raw_tap(1, capi.PAIR_TAP_POOL)  # no forward yet: no workspace
    net.forward(u8)
    for m, plane in ((capi.PAIR_TAP_POOL, capi.PAIR_TAP_PLANE_Q8), (0, 0), (capi.PAIR_TAP_INNER0 + 8, 0), (capi.PAIR_TAP_POOL, 2)):
        with pytest.raises(capi.HipacError):
            net.raw_tap(1, m, plane)  # fp16x3 has no byte tensor; unknown maps and planes
    with pytest.raises(capi.HipacError):
        net.raw_tap(2, capi.PAIR_TAP_POOL)  # more images than the last forward's workspace holds
    q8 = capi.PackedResNet18(sd, precision="fp16q8")
    q8.forward(u8)
    with pytest.raises(capi.HipacError):
        q8.raw_tap(1, capi.PAIR_TAP_BLOCK0 + 7, capi.PAIR_TAP_PLANE_Q8)  # the fp32 last map has no byte tensor
    lib = capi.load_library()
    dst = torch.empty(1 * 56 * 56 * 64 * 4, dtype=torch.uint8, device="cuda")
    args = lambda h, n_bytes: (h, net._ws.data_ptr(), 1, capi.PAIR_TAP_POOL, 0, dst.data_ptr(), n_bytes, None)  # noqa: E731
    assert lib.hipac_pair_tap_copy(*args(net.handle, dst.numel() - 1)) == -1 and b"dst holds" in lib.hipac_last_error()
    # more images than one sub-batch holds (HIPAC_SUBBATCH, 512 by default): refused before the workspace is looked at
    big = lib.hipac_pair_tap_bytes(513, capi.PRECISIONS["fp16x3"], capi.PAIR_TAP_POOL, 0)
    assert big == 513 * 56 * 56 * 64 * 4
    assert lib.hipac_pair_tap_copy(net.handle, net._ws.data_ptr(), 513, capi.PAIR_TAP_POOL, 0, dst.data_ptr(), big, None) == -1
    assert b"exceeds one sub-batch" in lib.hipac_last_error()
    assert lib.hipac_pair_tap_copy(net.handle, net._ws.data_ptr(), 0, capi.PAIR_TAP_POOL, 0, dst.data_ptr(), dst.numel(), None) == -1
    bf = capi.PackedResNet18(sd, precision="bf16")
    bf.forward(u8)
    assert lib.hipac_pair_tap_copy(*args(bf.handle, dst.numel())) != 0 and b"no pair mode" in lib.hipac_last_error()
    with pytest.raises(capi.HipacError):
        bf.raw_tap(1, capi.PAIR_TAP_POOL)
    assert lib.hipac_pair_tap_copy(*args(net.handle, dst.numel())) == 0  # and the same call with the right handle and size copies
    torch.cuda.synchronize()
    assert torch.equal(dst.view(1, 56, 56, 256), net.raw_tap(1, capi.PAIR_TAP_POOL))
