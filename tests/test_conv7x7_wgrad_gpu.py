"""The 7x7 stride-2 stem weight gradient (conv7x7_wgrad.hip) and its route
(GPU). Integer operands make the fp32 result bit-equal to the fp64 reference
in any summation order (tiles, partial rows, fold)."""
import functools

import pytest
import torch

import _mfma_exact_common as X

pytestmark = pytest.mark.gpu

# the forward's shapes (tests/test_conv7x7_gpu.py); the first has 8 tiles:
# max_blocks 3 = three trips per block with the accumulators carried across
# tiles, 1 = a single partial row
SHAPES = [(2, 3, 37, 41), (1, 3, 64, 64), (2, 3, 13, 9), (1, 1, 33, 35),
          (2, 4, 18, 22)]
EXACT = [(s, 0) for s in SHAPES] + [(SHAPES[0], 3), (SHAPES[0], 1)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e():
    from edl_amd import ops

    return ops.ext()


def _cl(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _dw64(x, dy):
    return torch.nn.grad.conv2d_weight(
        x.double(), (64, x.shape[1], 7, 7), dy.double(), stride=(2, 2),
        padding=(3, 3))


def _out(shape):
    n, _, h, w = shape
    return n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def _case(shape):
    """x, dy2d on the GPU and the fp64 reference: computed once, never
    written."""
    gen = torch.Generator().manual_seed(7749 + 5 * shape[2] + shape[3])
    x = X.ints(shape, X.ASYM3, gen)
    dy = X.ints(_out(shape), X.PM12, gen)
    ref = _dw64(x, dy)
    n, _, ho, wo = dy.shape
    X.check_budget(ref, n * ho * wo, x, dy, bf16_out=False)
    return _cl(x), X.rows(dy).contiguous().cuda(), ref


@pytest.mark.parametrize("shape,max_blocks", EXACT)
def test_exact(shape, max_blocks):
    x, dy2d, ref = _case(shape)
    X.check_exact(_e().conv7x7s2_wgrad(x, dy2d, max_blocks), ref, str(shape))


def _real(seed, shape=(2, 3, 64, 64)):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen).to(torch.bfloat16)
    dy = torch.randn(_out(shape), generator=gen).to(torch.bfloat16)
    return x, dy, _dw64(x, dy), _dw64(x.abs(), dy.abs())


def test_real_valued():
    x, dy, ref, absprod = _real(78)
    got = _e().conv7x7s2_wgrad(_cl(x), X.rows(dy).contiguous().cuda())
    ratio = X.bound_ratio(got, ref, absprod, 2 * 32 * 32)
    print(f"\nconv7x7 wgrad randn err/bound: {ratio:.4f}")
    assert ratio <= 1.0


def test_module_route(monkeypatch):
    import edl_amd.ops.conv as conv_mod
    from edl_amd.ops.conv import Conv2dFast

    calls = []
    real = _e().conv7x7s2_wgrad
    monkeypatch.setattr(_e(), "conv7x7s2_wgrad",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(2)
    conv = Conv2dFast(3, 64, 7, stride=2, padding=3, bias=False).cuda().train()
    x, dy, ref, absprod = _real(79)
    for on in (True, False):  # off: the library's line, no further call
        monkeypatch.setattr(conv_mod, "_CONV7X7_WGRAD", on)
        conv.weight.grad = None
        with torch.autocast("cuda", torch.bfloat16):
            conv(_cl(x.float())).backward(dy.cuda())
        assert len(calls) == 1
        g = conv.weight.grad
        assert g.dtype == conv.weight.dtype and g.shape == conv.weight.shape
        if on:
            assert X.bound_ratio(g, ref, absprod, 2 * 32 * 32) <= 1.0


# name: (the argument it replaces, from the good one, what the message says)
BAD = {
    "x fp32": ("x", lambda x: x.float(), "bf16"),
    "Cin 5": ("x", lambda x: _cl(torch.zeros(2, 5, 13, 9).bfloat16()), "Cin"),
    "dy2d rows": ("dy2d", lambda d: d[:-1], "rows"),
    "dy2d strided": ("dy2d", lambda d: torch.cat([d, d], 1)[:, ::2],
                     "contiguous"),
    "dy2d on the CPU": ("dy2d", lambda d: d.cpu(), "device"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_refusals(name):
    x, dy2d, _ = _case(SHAPES[2])
    a = dict(x=x, dy2d=dy2d)
    key, make, match = BAD[name]
    a[key] = make(a[key])
    with pytest.raises(RuntimeError, match=match):
        _e().conv7x7s2_wgrad(a["x"], a["dy2d"])
