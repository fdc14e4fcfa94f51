"""oracle/infer_replay.py pinned on torch itself, on the CPU.

(a) Unrounded, chained from the input, the replay IS the network: with storage None it equals
    oracle.resnet18_ref.resnet18_forward evaluated in float64 at every tap, to 1e-10 norm-relative (fold-then-conv against
    conv-then-BN) -- the fold, the geometry, the strip stem's bias-table algebra, the projection and its summed bias.
(b) A correct stand-in passes: tests/infer_replay_cases.py emulates the device with torch float32 convolutions and the
    device's rounding sites; every stage of every form must pass.  The printed figures show what the reference arithmetic
    alone uses of the bounds on exactly these inputs.
(c) Teeth: the same stand-in with one fault at a time (the list is in infer_replay_cases) must FAIL at the faulty stage,
    which passes without the fault.  The faults that change values (a dropped tap, swapped channels, a missing projection
    bias, the bias table's padding, the two head faults) put elements OUTSIDE their derived interval.  An unrounded inner map
    and a block output rounded towards zero are errors of the size of the rounding noise: with the worst-case term K e S they
    leave every element inside (in fp16 also with 4 sqrt(K) e S in its place: tried), and are caught by the block's mean-square
    statistic (the oracle's docstring) -- the unrounded inner map in bf16 at every block, in fp16 in layers 1 and 2, which is
    where the device could have it (layer1's fused block keeps the inner map on chip).

Stand-in figures here, 2 border patches, plain / rescaled weights, worst stage of each kind (the ratio of stem, features and
logits and the blocks' msq are asserted; a block's interval ratio is 1.000 whenever a device value sits on an end of its
interval, which grid values do; fig and sqrtK are reported, see the oracle's docstring):
            stem     block fig  block sqrtK  block msq    feats (split sum / head_kernel)  logits
  bf16      0.990    1.10       9.4          0.83 - 0.92  0.52 / 0.10                      6e-4
  fp16      0.946    0.87       2.4          0.46 - 0.75  0.51                             7e-4
  fp32      0.038    2.7e-4     0.06         0            0.11                             5e-4
"""
import pytest
import torch

import infer_replay_cases as cases
from oracle import infer_replay as IR, resnet18_ref as R

TAPS = ["stem", "maxpool"] + list(IR.BLOCKS)


@pytest.fixture(scope="module")
def u8():
    return cases.patches(2)


@pytest.fixture(scope="module")
def folded():
    cache = {}

    def get(kind, prec):
        if (kind, prec) not in cache:
            cache[(kind, prec)] = IR.fold(cases.state_dict(kind), IR.STORAGE[prec] if prec else None)
        return cache[(kind, prec)]
    return get


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("kind,form", [("plain", "u8_strip"), ("plain", "u8_table"), ("plain", "nchw_f32"), ("rescaled", "u8_strip")])
def test_unrounded_replay_is_the_float64_oracle(u8, folded, kind, form):
    x64 = cases.normalized64(u8)
    taps = {}
    ref_f, ref_l = R.resnet18_forward(x64, cases.state_dict(kind), taps, dtype=torch.float64)
    assert ref_f.dtype == torch.float64
    m = IR.replay_forward(x64 if form == "nchw_f32" else u8, folded(kind, None), None, stem=form)
    got = dict(zip(TAPS, [m["stem"], m["pool"]] + m["blocks"]), feats=m["feats"], logits=m["logits"])
    ref = dict({n: taps[n] for n in TAPS}, feats=ref_f, logits=ref_l)
    figures = {n: _rel(got[n], ref[n]) for n in ref}
    print(kind, form, {n: f"{v:.1e}" for n, v in figures.items()})
    assert all(v <= 1e-10 for v in figures.values()), figures


def test_strip_table_has_the_packers_classes():
    """Entry (0, 0) takes back 128 - 255 mean_c on all 147 taps; a class with taps outside differs from it by 255 mean_c per such tap."""
    rw = torch.randn(64, 3, 7, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    tab = IR.strip_table(rw, torch.zeros(64, dtype=torch.float64))
    mu = 255.0 * torch.tensor(IR.IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    assert torch.allclose(tab[0, 0], (rw * (128.0 - mu)).sum(dim=(1, 2, 3)), rtol=0, atol=1e-9)
    for cls, out_taps in ((1, [0, 1, 2]), (2, [0]), (3, [5, 6])):
        assert torch.allclose(tab[cls, 0] - tab[0, 0], (rw[:, :, out_taps, :] * mu).sum(dim=(1, 2, 3)), rtol=0, atol=1e-9)
        assert torch.allclose(tab[0, cls] - tab[0, 0], (rw[:, :, :, out_taps] * mu).sum(dim=(1, 2, 3)), rtol=0, atol=1e-9)


FORMS = [  # (precision, weights, stem form, fuse_stem, projk, pool_head)
    ("bf16", "plain", "u8_strip", True, True, True), ("fp16", "plain", "u8_strip", True, True, True),
    ("bf16", "rescaled", "u8_strip", True, True, True), ("fp16", "rescaled", "u8_strip", True, True, True),
    ("bf16", "plain", "u8_table", True, False, False), ("fp16", "plain", "nchw_f32", False, True, True),
    ("bf16", "plain", "nchw_f32", False, False, True), ("fp32", "plain", "nchw_f32", False, False, False),
    ("fp32", "rescaled", "nchw_f32", False, False, False)]


@pytest.mark.parametrize("prec,kind,form,fuse,projk,pool_head", FORMS)
def test_a_correct_stand_in_passes_every_stage(u8, folded, prec, kind, form, fuse, projk, pool_head):
    st, Fd = IR.STORAGE[prec], folded(kind, prec)
    inp = cases.normalized(u8) if form == "nchw_f32" else u8
    dev = cases.emulate(inp, Fd, st, stem=form, fuse_stem=fuse, projk=projk, pool_head=pool_head)
    res = IR.check_images(dev, range(2), Fd, st, stem=form, projk=projk, pool_head=pool_head)
    print(f"{prec} {kind} {form} fuse={fuse} projk={projk} pool_head={pool_head}\n{IR.summary(res)}")
    assert set(res) == ({"stem_pool"} if fuse and prec != "fp32" else {"stem", "pool"}) | set(IR.BLOCKS) | {"feats", "logits"}
    assert not IR.failures(res), IR.failures(res)


# ---------------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standin(folded):
    """The correct stand-in's maps, per precision: 2 patches through the whole net, 6 through it for the head faults."""
    cache = {}

    def get(prec, n):
        if (prec, n) not in cache:
            st, Fd = IR.STORAGE[prec], folded("plain", prec)
            u8 = cases.patches(n)
            form = "nchw_f32" if prec == "fp32" else "u8_strip"
            cache[(prec, n)] = cases.emulate(cases.normalized(u8) if prec == "fp32" else u8, Fd, st, stem=form)
        return cache[(prec, n)]
    return get


# (fault, block, what must see it).  "interval": elements outside the derived interval; "msq": the mean-square statistic -- an
# unrounded inner map and a mis-directed rounding are errors of the size of the rounding noise, which no worst case can see.
# The unrounded inner map sits where the device could have it: layer1's fused block keeps the inner map on chip, layer2.0 is
# the first block with its inner map in memory (fp16 from layer3 on: see the oracle's docstring).
BLOCK_FAULTS = [("drop_tap_col0", "layer1.0", "interval"), ("drop_tap_col0", "layer2.1", "interval"), ("drop_tap_col0", "layer4.1", "interval"),
                ("swap_channels", "layer3.1", "interval"), ("no_proj_bias", "layer2.0", "interval"), ("no_proj_bias", "layer4.0", "interval"),
                ("unrounded_inner", "layer1.0", "msq"), ("unrounded_inner", "layer1.1", "msq"), ("unrounded_inner", "layer2.0", "msq"),
                ("rtz_out", "layer1.0", "msq"), ("rtz_out", "layer3.1", "msq"), ("rtz_out", "layer4.0", "msq")]
# fp32: the stand-in's arithmetic IS float32, so there is no coarser rounding to leave out or to misdirect
BLOCK_CASES = [(p, f, b, how) for p in cases.PRECISIONS for f, b, how in BLOCK_FAULTS if not (p == "fp32" and how == "msq")]


@pytest.mark.parametrize("prec,fault,block,how", BLOCK_CASES)
def test_block_fault_is_caught_at_its_block(folded, standin, prec, fault, block, how):
    st, Fd, dev = IR.STORAGE[prec], folded("plain", prec), standin(prec, 2)
    i = IR.BLOCKS.index(block)
    X = dev["pool"] if i == 0 else dev["blocks"][i - 1]
    kind = IR.block_kind(block, st)
    good = IR.check_block(X, dev["blocks"][i], Fd[block], kind, st, last=i == 7)
    bad = IR.check_block(X, cases.emulate_block(X, Fd[block], kind, st, last=i == 7, fault=fault), Fd[block], kind, st, last=i == 7)
    gate = IR.msq_gate(bad["msq_n"])
    print(f"{prec} {fault} @ {block}: {bad['n_out']} elements outside, fig {bad['fig']:.3g}, sqrtK {bad['sqrtk']:.3g}, msq {bad['msq']:.3f} of gate "
          f"{gate:.3f} (without the fault: {good['n_out']} outside, fig {good['fig']:.3g}, sqrtK {good['sqrtk']:.3g}, msq {good['msq']:.3f})")
    assert not IR.failures({block: good})
    assert IR.failures({block: bad})
    if how == "interval":
        assert bad["ratio"] > 1.0 and bad["n_out"] > 0
    else:
        assert bad["msq"] > gate


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_strip_table_fault_is_caught_at_the_stem(folded, prec):
    st, Fd, u8 = IR.STORAGE[prec], folded("plain", prec), cases.patches(2)
    good = IR.check_stem("u8_strip", u8, Fd, st, cases.emulate_stem("u8_strip", u8, Fd, st)[1])["stem_pool"]
    bad = IR.check_stem("u8_strip", u8, Fd, st, cases.emulate_stem("u8_strip", u8, Fd, st, fault="pad_m128_last_row")[1])["stem_pool"]
    print(f"{prec}: {bad['n_out']} elements outside, worst {bad['worst']}, ratio {bad['ratio']:.3g}")
    assert good["n_out"] == 0 and bad["n_out"] > 0 and bad["ratio"] > 1.0
    assert bad["worst"][2] == 55  # only the last pooled row sees stem row 111


# (fp32 mode has no split-sum head)
HEAD_CASES = [(p, "half_wave", (2,)) for p in ("bf16", "fp16")] + [(p, "swap_3_4", (3, 4)) for p in cases.PRECISIONS]


@pytest.mark.parametrize("prec,fault,images", HEAD_CASES)
def test_head_fault_is_caught_at_the_features(folded, standin, prec, fault, images):
    Fd, dev = folded("plain", prec), standin(prec, 6)
    last, pool_head = dev["blocks"][7], prec != "fp32"
    f, l = cases.emulate_head(last, Fd["fc"], pool_head, fault=fault)
    good = IR.check_head(last, dev["feats"], dev["logits"], Fd["fc"], pool_head)
    bad = IR.check_head(last, f, l, Fd["fc"], pool_head)
    print(f"{prec} {fault}: features {bad['feats']['n_out']} outside, worst {bad['feats']['worst']}; logits {bad['logits']['n_out']} outside")
    assert good["feats"]["n_out"] == 0 and good["logits"]["n_out"] == 0
    assert bad["feats"]["ratio"] > 1.0 and bad["feats"]["worst"][0] in images
    assert bad["logits"]["n_out"] == 0  # the fc of the GIVEN features is still right: the fault is named at its own stage


def test_split_sum_precondition_is_asserted():
    last = torch.full((1, 512, 7, 7), 400.0, dtype=torch.float64)  # 49 x 400 > 2^14
    with pytest.raises(AssertionError):
        IR.check_head(last, last.mean(dim=(2, 3)), None, None, True)
