"""CPU, only where the reference tree exists: tests/resnetvd_ref.py (the fp32 restatement the GPU tests compare with) against
the reference's OWN ResNet of yolov7/modeling/backbone/resnetvd.py, loaded by path and constructed as its builder does -
state-dict keys and shapes (also of modeling/resnet_vd.ResNetVD), and on a one-block-per-stage net with shared weights the
outputs and every parameter gradient, at an even image and at one whose map is odd at every stride-2 step."""
import pytest
import torch

import ref_loader
import resnetvd_ref as V
from yolov7_d2_amd.modeling.resnet_vd import ResNetVD

pytestmark = pytest.mark.skipif(not ref_loader.available(), reason="the reference tree is not on this machine")


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize("layers", [(1, 1, 1, 1), (3, 4, 6, 3)], ids=["1111", "r50"])
def test_keys_and_shapes_equal_the_reference(layers):
    ref = _shapes(V.build_reference(layers).state_dict())
    mine = _shapes(V.ResNetVDRef(layers).state_dict())
    ours = _shapes(ResNetVD(layers).state_dict())
    assert list(ref) == list(mine) == list(ours)          # the same keys in the same order
    assert ref == mine == ours
    assert "conv1.6.weight" in ref and "layer2.0.downsample.1.weight" in ref and "layer1.0.downsample.2.running_var" in ref
    assert not any(k.startswith("layer1.0.downsample.0") for k in ref)


def test_zero_init_last_bn_and_default_conv_init_are_mirrored():
    ref, ours = V.build_reference((1, 1, 1, 1)), ResNetVD((1, 1, 1, 1))
    for net in (ref, ours):
        sd = net.state_dict()
        assert all(float(sd[f"layer{i}.0.bn3.weight"].abs().max()) == 0 for i in (1, 2, 3, 4))
        assert float(sd["layer1.0.bn2.weight"].min()) == 1 and float(sd["bn1.weight"].min()) == 1
        w = sd["layer3.0.conv2.weight"]                       # kaiming_uniform(a = sqrt(5)): |w| <= 1 / sqrt(fan_in)
        bound = (w.shape[1] * 9) ** -0.5 * (1 + 2 ** -23)       # (the fp32 draw may round up to the fp32 bound)
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound


@pytest.mark.parametrize("H,W", [(64, 96), (70, 90)])
def test_outputs_and_gradients_equal_the_reference(H, W):
    layers = (1, 1, 1, 1)
    ref, mine = V.build_reference(layers), V.ResNetVDRef(layers)
    sd = V.random_state(_shapes(mine.state_dict()), seed=7)
    ref.load_state_dict(sd)
    mine.load_state_dict(sd)
    g = torch.Generator().manual_seed(H)
    x = torch.randn(2, 3, H, W, generator=g)
    a, b = ref(x), mine(x)
    assert list(a) == list(b) == ["res3", "res4", "res5"]
    if H == 70:          # 35x45 after the stem convolutions, then 18x23, 9x12, 5x6, 3x3: odd at every stride-2 step
        assert tuple(b["res3"].shape[2:]) == (9, 12) and tuple(b["res4"].shape[2:]) == (5, 6) and tuple(b["res5"].shape[2:]) == (3, 3)
    cot = {k: torch.randn(v.shape, generator=g) for k, v in b.items()}
    sum((a[k] * cot[k]).sum() for k in a).backward()
    sum((b[k] * cot[k]).sum() for k in b).backward()
    for k in a:
        assert float((a[k] - b[k]).detach().norm() / a[k].detach().norm()) < 1e-5, k
    pa, pb = dict(ref.named_parameters()), dict(mine.named_parameters())
    assert list(pa) == list(pb) and len(pa) == 3 + 4 * 4
    for k in pa:
        assert float((pa[k].grad - pb[k].grad).norm() / pa[k].grad.norm()) < 1e-5, k
