"""Both native training steps (csrc/train.hip fp32, csrc/train_amp.hip fp16, the shared driver and small kernels of
csrc/train_common.h / train_kernels.h) STAGE BY STAGE against oracle/train_replay.py, through train_native.NativeEncoder.

tests/test_gpu_train.py and test_gpu_train_amp.py compare one whole step with an independent autograd graph, one number per
tensor; that stays the check that the driver is the right graph.  Here every stage is recomputed in float64 FROM THE DEVICE'S
OWN MAPS, rounded to the map type where the device rounds, so a stage is one rounding away from its reference and the backward
needs no activation pattern handed over (the masks are the device's maps).

Batches (the geometry is fixed at 224 x 224, so the batch is the only free size):
  B = 1   every tile, BN reduction pass and weight-gradient slice ends ragged (layer4: M = 49 pixels = one 32-pixel sub-chunk
          + 17, 13 reduction workgroups, the last with one row) -- compared, not only run
  B = 3   odd; layer4 has 147 pixels, layer1 73.5 weight-gradient slices
  B = 11  the fp16 stem and the four layer1 convs leave the 128-pixel weight-gradient chunk floor (192- and 160-pixel
          chunks), the fp32 stem its 256-pixel floor.  The wider layers leave the floor only from B >= 21: this test does NOT
          reach them.

(a) forward, stage-local: ``check_forward_stages`` -- per conv u |ref| + K e S, per BN the statistics at 2^-23, the running
    statistics at 2^-23, the normalisation at u |ref| + 8 e (...), the pool and its arg-max bit for bit, the features at
    50 e mean|v|; no element left out (bounds: oracle/train_replay.py).  Asserted: every ratio <= 1.
(b) backward, replayed: every gradient tensor against ``replay_backward`` of the device's maps in float64, max|a-b| / max|b|,
    and every conv weight also per filter tap [:, :, kh, kw] ("@tap": the worst tap).  Gate = 10 x the distance that float32
    accumulation leaves in the same replay on the CPU (tests/tools/measure_train_replay.py ->
    tests/golden/train_replay_distances.json, largest figure over the cases of the same precision; factor and rule of
    tests/test_gpu_mil_train.py).  dfeats = 2^k randn with the k recorded there.
(c) accumulate: two backwards on one forward, the second with accumulate = 1, against the sum of two replays; same gates.
(d) hipac_grads_unscale_check directly: inf / nan flagged wherever they sit, every finite float32 -- FLT_MAX included --
    passed and scaled exactly.

Measured on an MI355X.  (a), worst |given - ref| / bound of each kind of stage (must be <= 1; pool and arg-max: 0 differing
elements in every case):
              conv    mean/rstd  running  normalise  features
  fp32 B=1    0.067   0.499      0.495    0.362      0.099
  fp32 B=3    0.064   0.494      0.491    0.413      0.115
  fp32 B=11   0.073   0.493      0.495    0.391      0.112
  fp16 B=1    0.973   0.490      0.494    0.998      0.027
  fp16 B=3    0.974   0.494      0.495    0.999      0.034
  fp16 B=11   0.974   0.493      0.490    0.998      0.034
(the statistics are float32 roundings of float64 sums: half a unit of 2^-23; an fp16 map is dominated by its own rounding:
half a unit of u |ref|, so a stored value one fp16 unit off has ratio ~2.)
(b), (c): the tensor nearest to its gate, figure -> gate (10 x the CPU figure); every figure is printed by the test:
  fp32 B=1    layer4.0.bn1.bias     2.13e-6 -> 5.31e-6                              fp16 B=1    layer4.1.bn1.weight          2.30e-4 -> 9.05e-4
  fp32 B=3    layer4.0.bn1.weight   2.55e-6 -> 4.58e-6                               fp16 B=3    layer4.1.conv2.weight        8.32e-5 -> 5.16e-4
  fp32 B=11   layer4.0.bn2.weight   7.37e-7 -> 1.70e-6                               fp16 B=11   layer4.0.bn2.bias            5.65e-5 -> 4.17e-4
  fp32 B=3 accumulate  layer4.0.bn1.weight 1.92e-6 -> 4.58e-6                        fp16 B=3 accumulate  layer4.0.downsample.1.weight 1.12e-4 -> 6.93e-4
fp32 conv weights: 2e-7 ... 3.6e-6 (per tap up to 4.5e-6) against gates of 4e-6 ... 5e-5.  fp16: 4e-5 at layer4.1.conv2 rising to
1.3e-3 ... 1.8e-3 at layer1 and the stem (per tap up to 2.2e-3) against gates of 5e-4 rising to 1.6e-2 ... 2.1e-2 -- two float16 runs whose sums differ
in the last float32 bit decorrelate within a few rounded maps, so the float16 distance (device or CPU) is the format's rounding
noise carried through the backward, and the first tensors of the backward, which no rounded map precedes, are at 5e-8.
"""
import ctypes as C
import json
import os

import pytest
import torch

import train_stage_cases as cases
from oracle import train_replay as R
from ss25_hierarchical_multiscale_image_classification_amd import capi, train_native as TN

pytestmark = pytest.mark.gpu

FACTOR = 10.0
MEASURED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_replay_distances.json")))
GATES = MEASURED["per_storage"]

ALL_CASES = [(p, b) for p in ("fp32", "fp16") for b in cases.BATCHES]
ACC_CASES = [(p, cases.ACC_BATCH) for p in ("fp32", "fp16")]
_ids = lambda c: f"{c[0]}-B{c[1]}"  # noqa: E731


@pytest.fixture(scope="module")
def state_dict():
    return cases.make_state_dict()


@pytest.fixture(scope="module")
def case(request, state_dict):
    """One forward on the device and all its taps, copied back once (float32 holds an fp16 or fp32 map exactly)."""
    prec, batch = request.param
    enc = TN.NativeEncoder(state_dict, device="cuda", precision=prec)
    x = cases.make_input(batch)
    feats = enc.forward(x.cuda())
    torch.cuda.synchronize()
    maps = {"x": x, "feats": feats.cpu(), "pool": enc.tap(0, "pool", 0).cpu(), "pool_idx": enc.tap(0, "pool_idx", 0).cpu()}
    stats = enc.stats.cpu()
    for i, e in enumerate(enc.table):
        maps[("pre", i)], maps[("post", i)] = enc.tap(0, "pre", i).cpu(), enc.tap(0, "post", i).cpu()
        maps[("stats", i)] = tuple(t.cpu() for t in enc.tap(0, "stats", i))
        so, co = e["stat_off"], e["cout"]
        maps[("running", i)] = (stats[so:so + co], stats[so + co:so + 2 * co])
    return dict(prec=prec, batch=batch, storage=cases.STORAGE[prec], enc=enc, maps=maps, x=x, scale_exp=MEASURED["scale_exp"][str(batch)])


def _assert_gates(tag, prec, figures):
    print(tag, {k: f"{v:.2e}/{FACTOR * GATES[prec][k]:.2e}" for k, v in figures.items()})
    worst = max(figures, key=lambda k: figures[k] / GATES[prec][k])
    print(f"{tag}: worst {worst} {figures[worst]:.2e} of gate {FACTOR * GATES[prec][worst]:.2e}")
    bad = {k: (v, FACTOR * GATES[prec][k]) for k, v in figures.items() if not v <= FACTOR * GATES[prec][k]}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("case", ALL_CASES, indirect=True, ids=_ids)
def test_forward_every_stage_within_its_bound(case, state_dict):
    ratios = R.check_forward_stages(case["maps"], case["x"], state_dict, case["storage"], running=state_dict)
    assert len(ratios) == 4 * 20 + 3
    tag = f"{case['prec']}-B{case['batch']}"
    print(tag, {str(k): f"{v:.3f}" for k, v in ratios.items()})
    for kind in ("conv", "stats", "running", "bn"):
        print(f"{tag}: worst {kind} ratio {max(v for k, v in ratios.items() if isinstance(k, tuple) and k[0] == kind):.3f}")
    print(f"{tag}: pool {ratios['pool']}, pool_idx {ratios['pool_idx']}, feats {ratios['feats']:.3f}")
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("case", ALL_CASES, indirect=True, ids=_ids)
def test_backward_against_the_replay_of_the_devices_maps(case, state_dict):
    enc, batch = case["enc"], case["batch"]
    df = cases.make_dfeats(batch, case["scale_exp"])
    enc.backward(df.cuda())
    torch.cuda.synchronize()
    got = enc.state_dict(grads=True)
    ref = R.replay_backward(case["maps"], state_dict, df, case["storage"])
    assert set(got) == set(ref) and all(got[k].shape == ref[k].shape for k in ref)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    _assert_gates(f"{case['prec']}-B{batch}", case["prec"], cases.tensor_figures(got, ref))


@pytest.mark.parametrize("case", ACC_CASES, indirect=True, ids=_ids)
def test_accumulate_adds_a_second_backward(case, state_dict):
    """backward(df1, accumulate=False) then backward(df2, accumulate=True) on one workspace = replay(df1) + replay(df2): the
    second view of a SimCLR step through bn_bwd_apply_kernel and wgrad_reduce_kernel."""
    enc, batch = case["enc"], case["batch"]
    dfs = [cases.make_dfeats(batch, case["scale_exp"], w) for w in (0, 1)]
    enc.backward(dfs[0].cuda(), accumulate=False)
    enc.backward(dfs[1].cuda(), accumulate=True)
    torch.cuda.synchronize()
    got = enc.state_dict(grads=True)
    reps = [R.replay_backward(case["maps"], state_dict, df, case["storage"]) for df in dfs]
    ref = {k: reps[0][k] + reps[1][k] for k in reps[0]}
    _assert_gates(f"{case['prec']}-B{batch}-acc", case["prec"], cases.tensor_figures(got, ref))


FLT_MAX = 3.4028234663852886e38


def _unscale(values: torch.Tensor, inv_scale: float):
    g = values.clone().cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi._check(capi.load_library().hipac_grads_unscale_check(g.data_ptr(), g.numel(), C.c_float(inv_scale), flag.data_ptr(), capi._stream()),
                "hipac_grads_unscale_check")
    return g.cpu(), int(flag.item())


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_grads_unscale_check_flags_inf_and_nan_and_scales_the_rest_exactly(n):
    """Sizes around the 256-thread workgroup; one inf / -inf / nan first, last or in the middle -> the flag is 1 and every
    finite entry is still exactly fl(v * inv_scale); all finite -> the flag stays 0."""
    base = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 1000.0
    for inv_scale in (2.0 ** -10, 0.3):
        inv32 = torch.tensor(inv_scale, dtype=torch.float32)
        out, flag = _unscale(base, inv_scale)
        assert flag == 0 and torch.equal(out, base * inv32)
        for bad in (float("inf"), float("-inf"), float("nan")):
            for pos in sorted({0, n // 2, n - 1}):
                v = base.clone()
                v[pos] = bad
                out, flag = _unscale(v, inv_scale)
                keep = torch.arange(n) != pos
                assert flag == 1, (n, bad, pos)
                assert torch.equal(out[keep], (base * inv32)[keep]), (n, bad, pos)
                assert not bool(torch.isfinite(out[pos]))


def test_grads_unscale_check_passes_every_finite_float():
    """The header promises "inf / nan": a gradient between 3.0e38 and FLT_MAX is finite and must not skip the optimizer step
    (the kernel used to compare against 3.0e38).  A product that overflows IS inf and is flagged."""
    v = torch.tensor([1.0, 3.2e38, -3.3e38, FLT_MAX, -FLT_MAX, 0.0], dtype=torch.float32)
    out, flag = _unscale(v, 1.0)
    assert flag == 0 and torch.equal(out, v)
    out, flag = _unscale(v, 0.5)
    assert flag == 0 and torch.equal(out, v * 0.5)
    out, flag = _unscale(v, 2.0)
    assert flag == 1 and torch.equal(out, v * 2.0) and bool(torch.isinf(out[1]))
