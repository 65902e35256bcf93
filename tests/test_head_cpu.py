"""ops/head.py without a GPU: pool_linear is the two torch ops on CPU
tensors, and routing the models' heads through it leaves their state-dict
keys alone."""
import pytest
import torch
import torch.nn as nn

from edl_amd.ops.head import pool_linear


@pytest.mark.parametrize("bias", [True, False])
def test_pool_linear_cpu_is_the_torch_expression(bias):
    torch.manual_seed(0)
    fc = nn.Linear(64, 10, bias=bias)
    x = torch.randn(3, 64, 5, 4, requires_grad=True)
    want = fc(nn.AdaptiveAvgPool2d(1)(x).flatten(1))
    got = pool_linear(x, fc)
    assert torch.equal(got, want)
    gw, = torch.autograd.grad(want.sum(), x)
    gg, = torch.autograd.grad(got.sum(), x)
    assert torch.equal(gg, gw)


def test_models_keep_their_head_keys():
    from edl_amd.models.resnet_vd import resnet18_vd
    from edl_amd.models.resnext_wsl import ResNeXtWSL
    for m in (resnet18_vd(num_classes=4),
              ResNeXtWSL((1, 1, 1, 1), groups=2, base_width=4, num_classes=4)):
        keys = set(m.state_dict().keys())
        assert {"fc.weight", "fc.bias"} <= keys
        assert not any("head" in k or k.startswith("avgpool") for k in keys)
        assert isinstance(m.avgpool, nn.AdaptiveAvgPool2d)
        assert m.eval()(torch.randn(2, 3, 32, 32)).shape == (2, 4)
