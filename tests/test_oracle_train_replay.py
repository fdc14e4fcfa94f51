"""CPU: the stage-by-stage replay of the native training step (oracle/train_replay.py) pinned on torch itself.  With no
rounding (storage None) its forward must be the float64 forward of oracle/train_ref.py and its backward float64 autograd
of that graph; with a storage type the stage checker must accept the emulation's own maps and must name the one stage whose
map was disturbed.  These are the only trust tests/test_gpu_train_stages.py places in the replay."""
import pytest
import torch

from oracle import train_ref as TR
from oracle import train_replay as R
from oracle.resnet18_ref import canonical_state_dict
from ss25_hierarchical_multiscale_image_classification_amd.simclr import SimCLRModel


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = 0.5 + torch.rand(m.weight.shape, generator=g)
            m.bias.data = 0.1 * torch.randn(m.bias.shape, generator=g)
            m.running_mean.data = 0.1 * torch.randn(m.bias.shape, generator=g)
            m.running_var.data = 0.5 + torch.rand(m.bias.shape, generator=g)


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(29)
    model = SimCLRModel()
    _randomise_bn(model, 5)
    sd = canonical_state_dict({k: v.clone() for k, v in model.state_dict().items() if not k.startswith("projector.")})
    return sd, torch.randn(2, 3, 224, 224), torch.randn(2, 512)


@pytest.fixture(scope="module")
def f64_graph(setup):
    """float64 forward of oracle/train_ref.py with its taps, and float64 autograd of <feats, dfeats>."""
    sd, x, dfeats = setup
    p, stats = TR._split(sd, torch.float64)
    taps = {}
    feats = TR.encoder_train_forward(x.double(), p, stats, taps)
    (feats * dfeats.double()).sum().backward()
    return taps, feats.detach(), {k: v.grad for k, v in p.items() if v.grad is not None}, stats


def _maps_from_taps(taps, x):
    maps = {"x": x.double(), "pool": taps["pool"]}
    for i, e in enumerate(R.CONVS):
        maps[("pre", i)], maps[("post", i)] = taps[e["conv"] + ".pre"], taps[e["conv"] + ".post"]
        mean, var = R.batch_stats(maps[("pre", i)])
        maps[("stats", i)] = (mean, 1.0 / torch.sqrt(var + R.BN_EPS))
    maps["pool_idx"] = R.pool_first_max(maps[("post", 0)])[1]
    return maps


def test_conv_table_is_the_drivers():
    """Names, order and geometry of oracle.train_replay.CONVS against the library's own table."""
    from ss25_hierarchical_multiscale_image_classification_amd import train_native as TN

    table = TN.conv_table()
    assert len(table) == len(R.CONVS) == 20
    for a, b in zip(table, R.CONVS):
        assert all(a[k] == b[k] for k in ("conv", "bn", "cout", "cin", "ks", "stride")), (a, b)


def test_replay_backward_without_rounding_is_float64_autograd(setup, f64_graph):
    sd, x, dfeats = setup
    taps, _, grads_ref, _ = f64_graph
    got = R.replay_backward(_maps_from_taps(taps, x), sd, dfeats, None)
    assert set(got) == set(grads_ref)
    for k, g in grads_ref.items():
        err = float((got[k] - g).norm() / g.norm())
        assert got[k].shape == g.shape and err <= 1e-10, (k, err)


def test_emulate_forward_without_rounding_is_the_float64_forward(setup, f64_graph):
    sd, x, _ = setup
    taps, feats, _, stats = f64_graph
    maps = R.emulate_forward(x, sd, None, running=sd)
    ref = _maps_from_taps(taps, x)
    for i, e in enumerate(R.CONVS):
        for kind in ("pre", "post"):
            assert R.rel(maps[(kind, i)], ref[(kind, i)]) <= 1e-12, (kind, i)
        for a, b in zip(maps[("stats", i)], ref[("stats", i)]):
            assert R.rel(a, b) <= 1e-12, i
        # the running statistics against what F.batch_norm left in the float64 graph's buffers
        assert R.rel(maps[("running", i)][0], stats[e["bn"] + ".running_mean"]) <= 1e-12, i
        assert R.rel(maps[("running", i)][1], stats[e["bn"] + ".running_var"]) <= 1e-12, i
    assert R.rel(maps["pool"], ref["pool"]) <= 1e-12
    # the winners of two float64 forwards that differ by 1e-16 can differ only where a window holds a tie: all-zero windows
    differ = maps["pool_idx"] != ref["pool_idx"]
    assert not bool((maps["pool"][differ] != 0).any())
    assert R.rel(maps["feats"], feats) <= 1e-12


@pytest.fixture(scope="module", params=[torch.float32, torch.float16], ids=["float32", "float16"])
def emulated(request, setup):
    sd, x, _ = setup
    return request.param, R.emulate_forward(x, sd, request.param, running=sd)


def test_stage_checker_accepts_the_emulations_own_maps(setup, emulated):
    sd, x, _ = setup
    storage, maps = emulated
    ratios = R.check_forward_stages(maps, x, sd, storage, running=sd)
    assert len(ratios) == 4 * 20 + 3
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


def test_stage_checker_names_the_one_disturbed_stage(setup, emulated):
    """One element of pre[6] moved by 4 units in the last place of a float16 (the same relative step, 2^13 times as many
    units, in float32: the conv bound K e S of a float32 map is hundreds of ITS units wide): the conv that WROTE it is out
    of bound, and so are the two stages that READ it at a resolution of 2^-23 -- the batch statistics of that conv and the
    running statistics made from them, which move by 1 / M of the step.  Nothing else is: the element is one that the
    block's ReLU switches off, so the normalisation (checked with the GIVEN mean / rstd) still produces the given post[6],
    and no stage of any other conv sees the map."""
    sd, x, _ = setup
    storage, maps = emulated
    maps = dict(maps)
    pre = maps[("pre", 6)].clone()
    flat = pre.view(-1)
    off = maps[("post", 6)].view(-1) == 0
    j = int(torch.where(off, flat.abs(), torch.zeros_like(flat)).argmax())  # a normal number of either format
    ulp16 = 2.0 ** (torch.floor(torch.log2(flat[j].abs())) - 10)
    flat[j] += 4 * ulp16
    assert float(flat[j].to(storage).double()) == float(flat[j]) != float(maps[("pre", 6)].view(-1)[j])  # a value of the type
    maps[("pre", 6)] = pre
    ratios = R.check_forward_stages(maps, x, sd, storage, running=sd)
    bad = sorted((k for k, v in ratios.items() if not v <= 1.0), key=str)
    assert bad == [("conv", 6), ("running", 6), ("stats", 6)], {k: ratios[k] for k in bad}
