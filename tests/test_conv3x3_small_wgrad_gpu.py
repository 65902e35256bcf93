"""The small-channel 3x3 stem weight gradient (conv3x3_small_wgrad.hip) and
its route EDL_STEM_WGRAD=hip (GPU). Integer operands make the fp32 result
bit-equal to the fp64 reference in any summation order (k-steps over waves,
tiles, partial rows, fold). The kernel's tile is 16 x 16 output pixels."""
import functools

import pytest
import torch

import _mfma_exact_common as X

pytestmark = pytest.mark.gpu

# (N, Cin, Cout, H, W, stride). Per class: overhang both ways with 6 (narrow)
# / 8 (wide) tiles, one exact tile (narrow) / four (wide), a single
# overhanging tile per image, odd extents; Cin 1 / 3 / 4, both Cout.
NARROW = [(2, 3, 32, 37, 41, 2), (1, 3, 64, 64, 64, 2), (2, 1, 32, 13, 9, 2),
          (2, 4, 64, 18, 22, 2)]
WIDE = [(2, 32, 32, 19, 21, 1), (1, 32, 64, 32, 32, 1), (2, 32, 64, 13, 9, 1),
        (1, 32, 32, 33, 35, 1)]
# max_blocks 3 = several trips per block with the accumulators carried
# across tiles, 1 = a single partial row
EXACT = [(s, 0) for s in NARROW + WIDE] + [
    (s, mb) for s in (NARROW[0], WIDE[0]) for mb in (3, 1)]
REAL = {"narrow": (2, 3, 32, 64, 64, 2), "wide": (2, 32, 64, 32, 32, 1)}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e():
    from edl_amd import ops

    return ops.ext()


def _cl(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _shapes(shape):
    n, ci, co, h, w, s = shape
    return (n, ci, h, w), (n, co, (h - 1) // s + 1, (w - 1) // s + 1)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """x, dy2d on the GPU and the fp64 reference: computed once, never
    written."""
    xs, ys = _shapes(shape)
    gen = torch.Generator().manual_seed(3349 + 5 * shape[3] + shape[4])
    x = X.ints(xs, X.ASYM3, gen)
    dy = X.ints(ys, X.PM12, gen)
    ref = X.exact_ref_conv_dw(x, (shape[2], shape[1], 3, 3), dy, shape[5])
    k = ys[0] * ys[2] * ys[3]
    assert k <= 4096
    X.check_budget(ref, k, x, dy, bf16_out=False)
    return _cl(x), X.rows(dy).contiguous().cuda(), ref


@pytest.mark.parametrize("shape,max_blocks", EXACT)
def test_exact(shape, max_blocks):
    x, dy2d, ref = _case(shape)
    got = _e().conv3x3_small_wgrad(x, dy2d, shape[5], max_blocks)
    X.check_exact(got, ref, str(shape))


@functools.lru_cache(maxsize=None)
def _real(shape, seed):
    """randn operands rounded to bf16, the fp64 reference, |x| (*) |dy| and
    the bound's K (fp32 accumulation of K products, factor 2 for the tree)."""
    xs, ys = _shapes(shape)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(xs, generator=gen).to(torch.bfloat16)
    dy = torch.randn(ys, generator=gen).to(torch.bfloat16)
    ws = (shape[2], shape[1], 3, 3)
    return (x, dy, X.exact_ref_conv_dw(x, ws, dy, shape[5]),
            X.exact_ref_conv_dw(x.abs(), ws, dy.abs(), shape[5]),
            2 * ys[0] * ys[2] * ys[3])


@pytest.mark.parametrize("cls", list(REAL))
def test_real_valued(cls):
    shape = REAL[cls]
    x, dy, ref, absprod, k2 = _real(shape, 91)
    got = _e().conv3x3_small_wgrad(_cl(x), X.rows(dy).contiguous().cuda(),
                                   shape[5])
    ratio = X.bound_ratio(got, ref, absprod, k2)
    print(f"\nconv3x3 small wgrad {cls} randn err/bound: {ratio:.2e}")
    assert ratio <= 1.0


# (shape of the conv and its input, binding calls per backward under hip)
ROUTE = [(REAL["wide"], 1), (REAL["narrow"], 1), ((2, 48, 64, 16, 16, 1), 0)]


@pytest.mark.parametrize("shape,hip_calls", ROUTE)
def test_module_route(monkeypatch, shape, hip_calls):
    from edl_amd.ops.conv import Conv2dFast

    calls = []
    real = _e().conv3x3_small_wgrad
    monkeypatch.setattr(_e(), "conv3x3_small_wgrad",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(3)
    conv = Conv2dFast(shape[1], shape[2], 3, stride=shape[5], padding=1,
                      bias=False).cuda().train()
    x, dy, ref, absprod, k2 = _real(shape, 92)
    for route, want in (("hip", hip_calls), ("miopen", 0)):
        monkeypatch.setenv("EDL_STEM_WGRAD", route)
        conv.weight.grad = None
        del calls[:]
        with torch.autocast("cuda", torch.bfloat16):
            conv(_cl(x.float())).backward(dy.cuda())
        assert len(calls) == want
        g = conv.weight.grad
        assert g.dtype == conv.weight.dtype and g.shape == conv.weight.shape
        if want:
            assert X.bound_ratio(g, ref, absprod, k2) <= 1.0
        else:
            assert torch.isfinite(g).all() and g.abs().max() > 0


# name: (the argument it replaces, from the good one, stride, what the
# message says)
BAD = {
    "x fp32": ("x", lambda x: x.float(), 1, "x bf16"),
    "Cin 5": ("x", lambda x: _cl(torch.zeros(2, 5, 13, 9).bfloat16()), 1,
              "Cin, stride"),
    "Cin 32 stride 2": ("x", lambda x: x, 2, "Cin, stride"),
    "Cout 48": ("dy2d", lambda d: torch.cat([d, d], 1)[:, :48].contiguous(),
                1, "Cout"),
    "dy2d rows": ("dy2d", lambda d: d[:-1], 1, "rows"),
    "dy2d strided": ("dy2d", lambda d: torch.cat([d, d], 1)[:, ::2], 1,
                     "dy2d not contiguous"),
    "dy2d on the CPU": ("dy2d", lambda d: d.cpu(), 1, "dy2d on another device"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_refusals(name):
    x, dy2d, _ = _case(WIDE[2])
    a = dict(x=x, dy2d=dy2d)
    key, make, stride, match = BAD[name]
    a[key] = make(a[key])
    with pytest.raises(RuntimeError, match=match):
        _e().conv3x3_small_wgrad(a["x"], a["dy2d"], stride)
