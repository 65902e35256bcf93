"""conv_bn, the model call sites and the eval scale/shift cache, without a
GPU: on the CPU conv_bn is the two modules as written, the state-dict layout
of the models is what it was, and the cache follows the tensors it is built
from."""
import copy

import pytest
import torch

from edl_amd.models import resnet50_vd, resnext101_32x16d_wsl
from edl_amd.models.resnet_vd import BottleneckVd
from edl_amd.models.resnext_wsl import ResNeXtBottleneck
from edl_amd.ops.bnrelu import BNAddReLU2d, BNReLU2d
from edl_amd.ops.conv import Conv2dFast, conv_bn


def _randomize(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, BNReLU2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(
                    torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(
                    torch.rand(m.running_var.shape, generator=g) + 0.5)


@pytest.mark.parametrize("k,stride,groups", [(1, 1, 1), (1, 2, 1), (3, 1, 1),
                                             (3, 2, 4)])
@pytest.mark.parametrize("mode", ["eval", "eval_grad", "train"])
def test_conv_bn_cpu_is_the_two_modules(k, stride, groups, mode):
    torch.manual_seed(k + stride + groups)
    conv = Conv2dFast(64, 64, k, stride=stride, padding=k // 2, groups=groups,
                      bias=False)
    bn, bn_add = BNReLU2d(64, act=(k == 1)), BNAddReLU2d(64)
    _randomize(bn, 1)
    _randomize(bn_add, 2)
    x = torch.randn(2, 64, 9, 7)
    res = torch.randn(2, 64, *conv(x).shape[2:])
    for m in (conv, bn, bn_add):
        m.train(mode == "train")
    # training moves the running stats: each side gets its own copy
    bn2, bn_add2 = copy.deepcopy(bn), copy.deepcopy(bn_add)
    with torch.set_grad_enabled(mode != "eval"):
        assert torch.equal(conv_bn(conv, bn2, x), bn(conv(x)))
        assert torch.equal(conv_bn(conv, bn_add2, x, res),
                           bn_add(conv(x), res))
    for m, m2 in ((bn, bn2), (bn_add, bn_add2)):
        assert torch.equal(m.running_var, m2.running_var)
        assert m._batches_seen == m2._batches_seen == int(mode == "train")


@pytest.mark.parametrize("switch", [False, True])
def test_blocks_cpu_unchanged_by_the_switch(switch, monkeypatch):
    """Both blocks in eval on the CPU: the switch changes nothing there."""
    import edl_amd.ops.conv as conv_mod

    torch.manual_seed(0)
    blocks = [BottleneckVd(64, 16, stride=2), BottleneckVd(64, 16),
              ResNeXtBottleneck(64, 16, stride=2, groups=4, base_width=64),
              ResNeXtBottleneck(64, 16, groups=4, base_width=64)]
    x = torch.randn(2, 64, 8, 8)
    for i, blk in enumerate(blocks):
        _randomize(blk, 10 + i)
        blk.eval()
        monkeypatch.setattr(conv_mod, "_EVAL_FUSE", False)
        with torch.no_grad():
            want = blk(x)
        monkeypatch.setattr(conv_mod, "_EVAL_FUSE", switch)
        with torch.no_grad():
            assert torch.equal(blk(x), want)


def test_state_dict_keys_and_strict_load():
    with torch.device("meta"):  # the names only: no 194M-parameter init
        teacher = resnext101_32x16d_wsl(num_classes=10)
    keys = set(teacher.state_dict().keys())
    for name in ("stages.0.0.downsample.0.weight",
                 "stages.0.0.downsample.1.weight",
                 "stages.0.0.downsample.1.bias",
                 "stages.0.0.downsample.1.running_mean",
                 "stages.0.0.downsample.1.running_var",
                 "stages.0.0.downsample.1.num_batches_tracked",
                 "stages.1.0.downsample.0.weight",
                 "stages.3.0.downsample.1.running_mean",
                 "stages.0.0.conv1.weight", "stages.0.0.bn1.running_var",
                 "stages.2.22.conv3.weight", "stages.2.22.bn_add.weight"):
        assert name in keys, name
    assert not any(".downsample.conv" in k or ".downsample.bn" in k
                   for k in keys)
    assert "stages.0.1.downsample.0.weight" not in keys  # identity shortcut

    student = resnet50_vd(num_classes=10)
    skeys = set(student.state_dict().keys())
    for name in ("stages.0.0.conv0.conv.weight", "stages.0.0.conv0.bn.weight",
                 "stages.0.0.conv0.bn.running_mean",
                 "stages.0.0.conv1.conv.weight", "stages.0.0.conv2.weight",
                 "stages.0.0.bn_add.running_var",
                 "stages.0.0.shortcut.proj.conv.weight",
                 "stages.1.0.shortcut.proj.bn.running_mean",
                 "stem.0.conv.weight", "stem.0.bn.bias"):
        assert name in skeys, name

    # a state dict saved from one instance loads strictly into another
    small = dict(depths=(1, 1, 1, 1), groups=4, base_width=16, num_classes=4)
    from edl_amd.models.resnext_wsl import ResNeXtWSL

    a, b = ResNeXtWSL(**small), ResNeXtWSL(**small)
    _randomize(a, 3)
    assert b.load_state_dict(a.state_dict(), strict=True).missing_keys == []
    for (ka, va), (kb, vb) in zip(a.state_dict().items(),
                                  b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    s2 = resnet50_vd(num_classes=10)
    res = s2.load_state_dict(student.state_dict(), strict=True)
    assert res.missing_keys == [] and res.unexpected_keys == []


def _expected(bn):
    scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    return scale, bn.bias - bn.running_mean * scale


def test_eval_scale_shift_cache():
    bn = BNReLU2d(16)
    _randomize(bn, 4)
    with torch.no_grad():
        s0, t0 = bn.eval_scale_shift()
        for got, want in zip((s0, t0), _expected(bn)):
            assert torch.equal(got, want)
        s1, _ = bn.eval_scale_shift()
        assert s1 is s0  # served from the cache

        # an in-place update of running_var rebuilds it
        bn.running_var.mul_(4.0)
        s2, t2 = bn.eval_scale_shift()
        assert s2 is not s0 and not torch.equal(s2, s0)
        for got, want in zip((s2, t2), _expected(bn)):
            assert torch.equal(got, want)

        # a parameter replaced by a fresh tensor with EQUAL version counters:
        # only device/data_ptr() in the key can tell the two apart
        old = bn.weight
        fresh = torch.nn.Parameter(old.detach().clone() * 3.0)
        old_ver = old._version
        while fresh._version < old_ver:
            fresh.add_(0.0)
        assert fresh._version == old_ver
        bn.weight = fresh
        s3, t3 = bn.eval_scale_shift()
        assert not torch.equal(s3, s2)
        for got, want in zip((s3, t3), _expected(bn)):
            assert torch.equal(got, want)


def test_fused_eval_forward_uses_eval_scale_shift(monkeypatch):
    """_fused reads the cache through the method (one copy of the rule)."""
    bn = BNReLU2d(8)
    calls = []
    orig = BNReLU2d.eval_scale_shift

    def spy(self):
        calls.append(1)
        return orig(self)

    class _Ext:
        @staticmethod
        def bn_fwd_eval(x2d, scale, shift, res2d, relu):
            y = x2d.float() * scale + shift
            return (y.clamp(min=0) if relu else y).to(x2d.dtype)

    import edl_amd.ops.bnrelu as bn_mod

    monkeypatch.setattr(BNReLU2d, "eval_scale_shift", spy)
    monkeypatch.setattr(bn_mod, "ext", lambda: _Ext)
    bn.eval()
    x = torch.randn(2, 8, 3, 3).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    with torch.no_grad():
        y = bn._fused(x)
    assert calls == [1] and y.shape == x.shape
