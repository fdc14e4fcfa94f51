"""GPU: hipac_mil_forward against the fixtures the reference's own modules produced
(tests/golden/mil_golden.npz) and against the oracle on bags of many sizes.
fp32 everywhere; tolerance 2e-5 relative (summation order differs from torch's)."""
import os

import numpy as np
import pytest
import torch

from oracle import mil_ref
from ss25_hierarchical_multiscale_image_classification_amd import capi, mil

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    # two files, each under the 1 MiB a committed file may take: parameters + outputs, and the input bags
    return {**np.load(os.path.join(GOLD, "mil_golden.npz")), **np.load(os.path.join(GOLD, "mil_golden_bags.npz"))}


def sd_of(gold, pooling):
    pre = f"{pooling}.sd."
    return {k[len(pre):]: gold[k] for k in gold if k.startswith(pre)}


@pytest.mark.parametrize("pooling", ["attention", "mean", "max"])
def test_reference_fixtures_single_bag_and_batched(gold, pooling):
    m = mil.MILClassifier(512, num_classes=2, pooling=pooling)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_of(gold, pooling).items()})
    m = m.cuda().eval()
    bags = [torch.from_numpy(gold[f"bag{i}"]).cuda() for i in range(3)]
    for i, b in enumerate(bags):  # the reference's call shape: one bag per forward
        logits, attn = m(b)
        assert logits.shape == (2,)
        np.testing.assert_allclose(logits.cpu().numpy(), gold[f"{pooling}.logits{i}"], rtol=2e-5, atol=2e-6)
        if pooling == "attention":
            assert attn.shape == (b.shape[0], 1)
            np.testing.assert_allclose(attn.cpu().numpy(), gold[f"{pooling}.attn{i}"], rtol=2e-5, atol=1e-8)
        else:
            assert attn is None
    # all bags in one call
    offs = np.cumsum([0] + [b.shape[0] for b in bags])
    logits, attn, pooled = m.forward_bags(torch.cat(bags), offs, want_pooled=True)
    for i in range(3):
        np.testing.assert_allclose(logits[i].cpu().numpy(), gold[f"{pooling}.logits{i}"], rtol=2e-5, atol=2e-6)
        _, _, p_ref = mil_ref.mil_forward_ref(sd_of(gold, pooling), gold[f"bag{i}"], pooling)
        np.testing.assert_allclose(pooled[i].cpu().numpy(), p_ref, rtol=2e-5, atol=2e-6)


def test_many_ragged_bags_against_oracle(gold):
    sd = sd_of(gold, "attention")
    m = mil.MILClassifier(512, pooling="attention")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    rng = np.random.RandomState(0)
    sizes = [1, 2, 15, 16, 17, 255, 256, 257, 1000, 4133]
    feats = rng.randn(sum(sizes), 512).astype(np.float32) * 0.7
    offs = np.cumsum([0] + sizes)
    logits, attn = m.forward_bags(torch.from_numpy(feats).cuda(), offs)
    for i, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        l_ref, a_ref, _ = mil_ref.mil_forward_ref(sd, feats[a:b], "attention")
        np.testing.assert_allclose(logits[i].cpu().numpy(), l_ref, rtol=5e-5, atol=5e-6)
        np.testing.assert_allclose(attn[a:b].cpu().numpy(), a_ref[:, 0], rtol=1e-4, atol=1e-9)
        assert abs(float(attn[a:b].sum()) - 1.0) < 1e-4


def test_error_paths(gold):
    m = mil.MILClassifier(512).cuda().eval()
    x = torch.zeros(8, 512, device="cuda")
    with pytest.raises(capi.HipacError):
        m.forward_bags(x, [0, 3, 3, 8])  # empty bag
    with pytest.raises(capi.HipacError):
        m.forward_bags(x, [0, 7])        # does not cover all rows
    with pytest.raises(capi.HipacError):
        m.forward_bags(x.cpu(), [0, 8])
    with pytest.raises(capi.HipacError):
        m.forward_bags(x.double(), [0, 8])


@pytest.mark.parametrize("F,pooling", [(128, "attention"), (64, "max"), (1024, "mean")])
def test_other_feature_dims_against_oracle(F, pooling):
    # the head is not tied to 512-d ResNet18 features (the reference passes feature_dim)
    torch.manual_seed(F)
    m = mil.MILClassifier(F, num_classes=3, pooling=pooling).cuda().eval()
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    rng = np.random.RandomState(F)
    sizes = [3, 40, 129]
    feats = rng.randn(sum(sizes), F).astype(np.float32)
    offs = np.cumsum([0] + sizes)
    logits, attn = m.forward_bags(torch.from_numpy(feats).cuda(), offs)
    assert logits.shape == (3, 3)
    for i, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        l_ref, a_ref, _ = mil_ref.mil_forward_ref(sd, feats[a:b], pooling)
        np.testing.assert_allclose(logits[i].cpu().numpy(), l_ref, rtol=5e-5, atol=5e-6)
        if pooling == "attention":
            np.testing.assert_allclose(attn[a:b].cpu().numpy(), a_ref[:, 0], rtol=1e-4, atol=1e-9)
