"""The 7x7 stride-2 stem kernel (conv7x7.hip) and its routes (GPU). Integer
operands make the bf16 output bit-equal to the fp64 reference rounded once;
the fused epilogue is bit-equal to the plain kernel + bn_fwd_eval."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _mfma_exact_common as X
from _eval_affine_common import affine, affine_bound_ratio

pytestmark = pytest.mark.gpu

# (n, cin, h, w): odd H and W with a 5-wide fragment tail, a 3-row tile tail
# and two images; 2x2 exact tiles; smaller than one fragment; Cin 1; Cin 4
SHAPES = [(2, 3, 37, 41), (1, 3, 64, 64), (2, 3, 13, 9), (1, 1, 33, 35),
          (2, 4, 18, 22)]
# max_blocks 3 on the 8 tiles of the first shape: three trips of the
# persistent loop per block, both patch buffers in use
EXACT = [(s, 0) for s in SHAPES] + [(SHAPES[0], 3)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e():
    from edl_amd import ops

    return ops.ext()


def _cl(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _conv64(x, w):
    return F.conv2d(x.double(), w.double(), stride=2, padding=3)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """x, w7 (as ops/conv.py builds it), the fp64 conv rows: computed once,
    shared by the tests below, never written."""
    from edl_amd.ops.conv import _repack_w7

    n, cin, h, w = shape
    gen = torch.Generator().manual_seed(7700 + 5 * h + w + cin)
    x = X.ints(shape, X.PM12, gen)
    wt = X.ints((64, cin, 7, 7), X.ASYM3, gen)
    ref = X.rows(_conv64(x, wt)).contiguous()
    X.check_budget(ref, 49 * cin, x, wt, bf16_out=True)
    assert X.small_share(ref) >= 0.9
    return _cl(x), _repack_w7(wt.cuda()), ref


@pytest.mark.parametrize("shape,max_blocks", EXACT)
def test_exact(shape, max_blocks):
    x, w7, ref = _case(shape)
    X.check_exact(_e().conv7x7s2_fwd(x, w7, max_blocks), ref, str(shape))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_fused_epilogue(shape, relu):
    e = _e()
    x, w7, ref = _case(shape)
    scale, shift = affine(64, torch.Generator(device="cuda").manual_seed(
        shape[2] + relu))
    got = e.conv7x7s2_fwd_bn(x, w7, scale, shift, relu)
    want = e.bn_fwd_eval(e.conv7x7s2_fwd(x, w7), scale, shift, None, relu)
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape
    assert torch.equal(got, want)
    yb = ref.to(torch.bfloat16).double()
    ratio = affine_bound_ratio(got, yb, scale, shift, torch.zeros_like(yb),
                               relu)
    print(f"\nconv7x7 bn err/bound {shape} relu={relu}: {ratio:.4f}")
    assert ratio <= 1.0


def test_real_valued():
    from edl_amd.ops.conv import _repack_w7

    gen = torch.Generator().manual_seed(77)
    x = torch.randn(2, 3, 64, 64, generator=gen).to(torch.bfloat16)
    wt = torch.randn(64, 3, 7, 7, generator=gen).to(torch.bfloat16)
    ref = X.rows(_conv64(x, wt))
    absprod = X.rows(_conv64(x.abs(), wt.abs()))
    got = _e().conv7x7s2_fwd(_cl(x), _repack_w7(wt.cuda()))
    ratio = X.bound_ratio(got, ref, absprod, 147)
    print(f"\nconv7x7 randn err/bound: {ratio:.4f}")
    assert ratio <= 1.0


NAMES = ["conv7x7s2_fwd", "conv7x7s2_fwd_bn", "bn_fwd_eval"]


def _spy(monkeypatch):
    calls = dict.fromkeys(NAMES, 0)

    def wrap(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f

    for name in NAMES:
        monkeypatch.setattr(_e(), name, wrap(name, getattr(_e(), name)))
    return calls


def _stem(seed):
    from edl_amd.ops.bnrelu import BNReLU2d
    from edl_amd.ops.conv import Conv2dFast

    torch.manual_seed(seed)
    conv = Conv2dFast(3, 64, 7, stride=2, padding=3, bias=False).cuda()
    bn = BNReLU2d(64).cuda()
    with torch.no_grad():
        for t in (bn.weight, bn.bias, bn.running_mean):
            t.copy_(torch.randn(64))
        bn.running_var.copy_(torch.rand(64) + 0.5)
    x = torch.randn(2, 3, 30, 34).to(torch.bfloat16)
    return conv, bn, _cl(x)


def test_module_route(monkeypatch):
    import edl_amd.ops.conv as conv_mod

    conv, _, xb = _stem(1)
    conv.to(torch.bfloat16)
    calls = _spy(monkeypatch)
    yb = conv(xb)
    assert calls["conv7x7s2_fwd"] == 1 and yb.shape == (2, 64, 15, 17)
    conv.float()
    with torch.autocast("cuda", torch.bfloat16):
        y32 = conv(xb.float())
        assert calls["conv7x7s2_fwd"] == 2 and torch.equal(y32, yb)
        conv(xb.float().requires_grad_(True))
        monkeypatch.setattr(conv_mod, "_CONV7X7", False)
        conv(xb.float())
        assert calls == {NAMES[0]: 2, NAMES[1]: 0, NAMES[2]: 0}
        # train(): the forward in-repo, the weight gradient the library's
        monkeypatch.setattr(conv_mod, "_CONV7X7", True)
        conv.train()(xb.float()).sum().backward()
    g = conv.weight.grad
    assert calls[NAMES[0]] == 3
    assert g.shape == conv.weight.shape and g.dtype == conv.weight.dtype
    assert torch.isfinite(g).all()


def test_conv_bn_one_kernel(monkeypatch):
    from edl_amd.ops.conv import conv_bn

    conv, bn, xb = _stem(3)
    conv.to(torch.bfloat16).eval()
    bn.eval()
    calls = _spy(monkeypatch)
    with torch.no_grad():
        got = conv_bn(conv, bn, xb)
        assert calls == {"conv7x7s2_fwd": 0, "conv7x7s2_fwd_bn": 1,
                         "bn_fwd_eval": 0}
        assert torch.equal(got, bn(conv(xb)))
    assert calls == {"conv7x7s2_fwd": 1, "conv7x7s2_fwd_bn": 1,
                     "bn_fwd_eval": 1}


def test_model_same_bits_with_and_without_eval_fuse(monkeypatch):
    import edl_amd.ops.conv as conv_mod
    from edl_amd.models.resnext_wsl import ResNeXtWSL

    torch.manual_seed(4)
    m = ResNeXtWSL((1, 1, 1, 1), groups=4, base_width=16, num_classes=4)
    m = m.cuda().to(memory_format=torch.channels_last).eval()
    x = _cl(torch.randn(2, 3, 64, 64))
    calls = _spy(monkeypatch)
    out = {}
    for on in (False, True):
        monkeypatch.setattr(conv_mod, "_EVAL_FUSE", on)
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            out[on] = m(x)
        assert calls["conv7x7s2_fwd"] == 1 and calls["conv7x7s2_fwd_bn"] == on
    assert torch.isfinite(out[True].float()).all()
    assert torch.equal(out[True], out[False])


def _z(*shape):
    return _cl(torch.zeros(*shape, dtype=torch.bfloat16))


# name: (the argument it replaces, from the good one, what the message says)
BAD = {
    "x fp32": ("x", lambda x: x.float(), "bf16"),
    "x 3-D": ("x", lambda x: x[0], "4-D"),
    "x not channels_last": ("x", lambda x: x.contiguous(), "channels_last"),
    "x on the CPU": ("x", lambda x: x.cpu(), "GPU"),
    "Cin 5": ("x", lambda x: _z(1, 5, 9, 9), "Cin"),
    "H 0": ("x", lambda x: _z(1, 3, 0, 9), "H, W"),
    "w7 fp32": ("w7", lambda w: w.float(), "bf16"),
    "w7 shape": ("w7", lambda w: w[:, :192].contiguous(), "shape"),
    "w7 strided": ("w7", lambda w: torch.cat([w, w], 1)[:, ::2], "contiguous"),
    "w7 unaligned": ("w7", lambda w: torch.cat(
        [w.flatten()[:1], w.flatten()])[1:].view(64, 224), "aligned"),
    "scale fp64": ("scale", lambda t: t.double(), "fp32"),
    "shift shape": ("shift", lambda t: t[:-1], "shape"),
    "scale strided": ("scale", lambda t: torch.cat([t, t])[::2], "contiguous"),
    "shift on the CPU": ("shift", lambda t: t.cpu(), "device"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_refusals(name):
    x, w7, _ = _case(SHAPES[2])
    scale, shift = affine(64, torch.Generator(device="cuda").manual_seed(5))
    a = dict(x=x, w7=w7, scale=scale, shift=shift)
    key, make, match = BAD[name]
    a[key] = make(a[key])
    with pytest.raises(RuntimeError, match=match):
        _e().conv7x7s2_fwd_bn(a["x"], a["w7"], a["scale"], a["shift"], True)
    if key in ("x", "w7"):
        with pytest.raises(RuntimeError, match=match):
            _e().conv7x7s2_fwd(a["x"], a["w7"])
