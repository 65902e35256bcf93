"""Inference forward with conv -> BN(+Add)+ReLU pairs in one kernel (GPU).

ops.conv.conv_bn takes the fused bindings exactly where the unfused path
runs both in-repo kernels, and they are bit-equal to that pair, so blocks
and models give the same bits under EDL_EVAL_FUSE 0 and 1 wherever the route
itself is deterministic (every 1x1, the grouped 3x3, dense 3x3 non-split or
with two split-K slices: a + b in either order)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

FUSED = ["gemm_bt_bn", "conv3x3_fwd_bn_padded", "conv3x3_grouped_fwd_bn"]
UNFUSED = ["bn_fwd_eval", "gemm_bt", "conv3x3_fwd_padded", "conv3x3_fwd",
           "conv3x3_grouped_fwd"]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class _Spy:
    """Counts calls of the extension's entry points by name."""

    def __init__(self, monkeypatch, names):
        from edl_amd import ops

        self.calls = {n: 0 for n in names}
        e = ops.ext()
        for n in names:
            monkeypatch.setattr(e, n, self._wrap(n, getattr(e, n)))

    def _wrap(self, name, fn):
        def f(*a, **k):
            self.calls[name] += 1
            return fn(*a, **k)

        return f

    def reset(self):
        for n in self.calls:
            self.calls[n] = 0


def _set_fuse(monkeypatch, on):
    import edl_amd.ops.conv as conv_mod

    monkeypatch.setattr(conv_mod, "_EVAL_FUSE", on)


def _randomize_bn(mod, seed):
    """Non-trivial affine parameters and running statistics."""
    from edl_amd.ops.bnrelu import BNReLU2d

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, BNReLU2d):
                c = m.num_features
                m.weight.copy_(torch.randn(c, generator=g))
                m.bias.copy_(torch.randn(c, generator=g))
                m.running_mean.copy_(torch.randn(c, generator=g))
                m.running_var.copy_(torch.rand(c, generator=g) + 0.5)


def _int_input(c, seed, hw=14):
    """Integer-valued bf16 channels_last [2, c, hw, hw]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (2, c, hw, hw), generator=g).to(torch.bfloat16)
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _resnext_block(cin, stride):
    from edl_amd.models.resnext_wsl import ResNeXtBottleneck

    torch.manual_seed(40 + cin + stride)
    blk = ResNeXtBottleneck(cin, 64, stride=stride).cuda().eval()
    _randomize_bn(blk, cin + stride)
    return blk


def _vd_block(cin, stride, if_first=False):
    from edl_amd.models.resnet_vd import BottleneckVd

    torch.manual_seed(50 + cin + stride)
    blk = BottleneckVd(cin, 64, stride=stride, if_first=if_first).cuda().eval()
    _randomize_bn(blk, 7 * cin + stride)
    return blk


# block, input channels, expected fused calls under EDL_EVAL_FUSE=1:
# (gemm_bt_bn, conv3x3_fwd_bn_padded, conv3x3_grouped_fwd_bn)
BLOCKS = {
    # planes 64: width 512 (cpg 16), cout 256
    "resnext-identity": (lambda: _resnext_block(256, 1), 256, (2, 0, 1)),
    "resnext-down-s1": (lambda: _resnext_block(64, 1), 64, (3, 0, 1)),
    "resnext-down-s2": (lambda: _resnext_block(256, 2), 256, (3, 0, 1)),
    # conv1 is a dense 64 -> 64 3x3: M 392 / 98, two split-K slices
    "vd-identity": (lambda: _vd_block(256, 1), 256, (2, 1, 0)),
    "vd-first": (lambda: _vd_block(64, 1, True), 64, (3, 1, 0)),
    "vd-pool-s2": (lambda: _vd_block(256, 2), 256, (3, 1, 0)),
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_eval_bit_equal_and_routed(name, monkeypatch):
    make, cin, want_calls = BLOCKS[name]
    blk = make()
    x = _int_input(cin, 60 + cin)
    spy = _Spy(monkeypatch, FUSED + UNFUSED)

    _set_fuse(monkeypatch, False)
    with torch.no_grad():
        want = blk(x)
    assert all(spy.calls[n] == 0 for n in FUSED), spy.calls
    assert spy.calls["bn_fwd_eval"] == sum(want_calls)  # one per pair

    spy.reset()
    _set_fuse(monkeypatch, True)
    with torch.no_grad():
        got = blk(x)
    assert tuple(spy.calls[n] for n in FUSED) == want_calls, spy.calls
    assert all(spy.calls[n] == 0 for n in UNFUSED), spy.calls
    assert got.dtype == torch.bfloat16 and got.shape == want.shape
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert bool(got.float().abs().sum() > 0)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["resnext-down-s2", "vd-pool-s2"])
def test_block_autograd_on_takes_no_fused_binding(name, monkeypatch):
    """eval() but autograd on (a frozen block: its grouped conv keeps the
    in-repo route): the pairs stay two calls, as on the parent."""
    make, cin, _ = BLOCKS[name]
    blk = make()
    for p in blk.parameters():
        p.requires_grad_(False)
    x = _int_input(cin, 70 + cin)
    spy = _Spy(monkeypatch, FUSED)
    outs = []
    for on in (False, True):
        _set_fuse(monkeypatch, on)
        with torch.enable_grad():
            outs.append(blk(x))
    assert all(v == 0 for v in spy.calls.values()), spy.calls
    assert torch.equal(outs[0], outs[1])


def test_block_train_mode_takes_no_fused_binding(monkeypatch):
    """train(): the training forward and backward are the parent's."""
    from edl_amd.ops.conv import Conv2dFast

    blk0 = _vd_block(256, 2).train()
    for m in blk0.modules():
        if isinstance(m, Conv2dFast):
            m.to(torch.bfloat16)
    spy = _Spy(monkeypatch, FUSED)
    res = []
    for on in (False, True):
        _set_fuse(monkeypatch, on)
        blk = copy.deepcopy(blk0)
        x = _int_input(256, 80).requires_grad_(True)
        y = blk(x)
        y.float().square().mean().backward()
        res.append((y.detach(), blk.bn_add.running_var.clone(), x.grad))
    assert all(v == 0 for v in spy.calls.values()), spy.calls
    (y0, rv0, dx0), (y1, rv1, dx1) = res
    assert torch.equal(y0, y1) and torch.equal(rv0, rv1)
    # the BN backward reduces with atomics: the tolerance the padded-fusion
    # tests use for the same block's input gradient
    assert torch.allclose(dx0.float(), dx1.float(), atol=1e-2, rtol=1e-2)


def _logits(model, x):
    # as the trainer's evaluate and the teacher server run a model: fp32
    # parameters, bf16 autocast
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        return model(x).float()


@pytest.mark.parametrize("arch", ["resnet18_vd", "resnet50_vd"])
def test_model_eval_logits(arch, monkeypatch):
    """Both nets have dense 3x3s with FOUR or more split-K slices at this
    size (128 -> 128 at 8x8: one tile, KT 18), whose fp32 atomics arrive in
    any order, so the unfused forward need not repeat itself bit for bit.
    The fused forward is compared within that run-to-run difference,
    measured here on three unfused runs: 4x the largest pairwise difference,
    and, where the three happen to agree, 4 bf16 ulps (2^-8 relative) of the
    largest logit, the size of a few flipped roundings."""
    from edl_amd import models

    torch.manual_seed(90)
    model = getattr(models, arch)(num_classes=10).cuda()
    _randomize_bn(model, 91)
    model = model.to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(92)
    x = torch.randn(2, 3, 64, 64, generator=g).cuda().contiguous(
        memory_format=torch.channels_last)
    spy = _Spy(monkeypatch, FUSED + ["bn_fwd_eval"])

    _set_fuse(monkeypatch, False)
    base = [_logits(model, x) for _ in range(3)]
    assert all(spy.calls[n] == 0 for n in FUSED)
    n_bn = spy.calls["bn_fwd_eval"] // 3
    floor = max((base[i] - base[j]).abs().max().item()
                for i in range(3) for j in range(i))
    spy.reset()
    _set_fuse(monkeypatch, True)
    got = _logits(model, x)
    fused = sum(spy.calls[n] for n in FUSED)
    # every BN is behind a conv; the three stem BNs (small-channel kernel)
    # and each BasicBlock tail (a 3x3 with a residual) keep their launch
    assert fused > 0 and fused + spy.calls["bn_fwd_eval"] == n_bn
    tails = {"resnet18_vd": 8, "resnet50_vd": 0}[arch]
    assert spy.calls["bn_fwd_eval"] == 3 + tails
    assert torch.isfinite(got).all()
    diff = (got - base[0]).abs().max().item()
    bound = max(4 * floor, 4 * 2.0 ** -8 * base[0].abs().max().item())
    print(f"\neval fuse {arch}: floor={floor:.3e} diff={diff:.3e} "
          f"bound={bound:.3e} fused pairs={fused} of {n_bn}")
    assert diff <= bound


class _FixedLoader:
    def __init__(self, batches):
        self.batches = batches
        self.i = 0

    def next(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        return b


def test_engine_evaluate_same_under_both_settings(monkeypatch):
    from edl_amd.train.engine import TrainerEngine

    eng = TrainerEngine(model="resnet18_vd", per_device_batch=8,
                        num_classes=10, dtype="bf16", base_lr=0.05,
                        use_hip_ops=True, checkpoint_dir=None,
                        graph_capture=False).setup()
    g = torch.Generator().manual_seed(5)
    batches = []
    for _ in range(2):
        x = torch.randn(8, 3, 64, 64, generator=g).cuda().contiguous(
            memory_format=torch.channels_last)
        batches.append((x, torch.randint(0, 10, (8,), generator=g).cuda()))
    spy = _Spy(monkeypatch, FUSED)
    out = []
    for on in (False, True):
        _set_fuse(monkeypatch, on)
        out.append(eng.evaluate(_FixedLoader(batches), 2))
        assert (sum(spy.calls.values()) > 0) == on
    print("\neval fuse evaluate:", out)
    assert out[0]["samples"] == out[1]["samples"] == 16
    assert out[0]["acc1"] == out[1]["acc1"]
