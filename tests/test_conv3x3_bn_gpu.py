"""The 3x3 kernels with the eval BN(+ReLU) apply behind them (GPU).

conv3x3_fwd_bn_padded and conv3x3_grouped_fwd_bn return what the plain conv
binding followed by bn_fwd_eval returns, bit for bit: non-split dense shapes
and every grouped shape run the affine in the kernel epilogue, split-K dense
shapes run the split-K launch, the cast and the BN apply kernel inside the
binding. x and w are integers, so the convolution is exact in any
accumulation order and the more-than-two-slice split-K route (fp32 atomics
in arrival order) is deterministic too.

Routes, from conv3x3_pick_splitk (docs/kernels.md route table):
  (2, 64, 9, 11) -> 64    s1, s2   2 slices
  (1, 256, 7, 7) -> 128   s1       9 slices
  (2, 64, 79, 79) -> 256  s1       non-split: the fused epilogue"""
import functools

import pytest
import torch

import _mfma_exact_common as X
from _eval_affine_common import affine, affine_bound_ratio

pytestmark = pytest.mark.gpu

# (n, ci, h, w, co), stride, split-K slices
DENSE = [((2, 64, 9, 11, 64), 1, 2),
         ((2, 64, 9, 11, 64), 2, 2),
         ((1, 256, 7, 7, 128), 1, 9),
         ((2, 64, 79, 79, 256), 1, 1)]
GROUPED = [(cpg, stride) for cpg in (16, 64) for stride in (1, 2)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e():
    from edl_amd import ops

    return ops.ext()


def _cl(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _affine(n, seed):
    return affine(n, torch.Generator(device="cuda").manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _dense_case(shape, stride):
    """x, w3 (as ops/conv.py builds it), the fp64 conv rows: computed once,
    shared by the tests below, never written."""
    from edl_amd.ops.conv import _repack_w3

    n, ci, h, w, co = shape
    gen = torch.Generator().manual_seed(9000 + ci + 3 * h + 7 * co + stride)
    x = X.ints((n, ci, h, w), X.PM12, gen)
    wt = X.ints((co, ci, 3, 3), X.PM1, gen)
    ref = X.rows(X.exact_ref_conv(x, wt, stride)).contiguous()
    X.check_budget(ref, 9 * ci, x, wt, bf16_out=True)
    assert X.small_share(ref) >= 0.9
    return _cl(x), _repack_w3(wt.cuda()), ref


@functools.lru_cache(maxsize=None)
def _grouped_case(cpg, stride):
    """The shapes of test_conv3x3_grouped_fwd_exact: cpg 16 is the
    block-diagonal repack (gw 64), cpg 64 the per-group dense one."""
    from edl_amd.ops.conv import _repack_w3_grouped

    C = 2 * max(cpg, 32)
    gen = torch.Generator().manual_seed(9500 + cpg + stride)
    x = X.ints((1, C, 7, 9), X.PM12, gen)
    wt = X.ints((C, cpg, 3, 3), X.ASYM3, gen)
    ref = X.rows(X.exact_ref_conv(x, wt, stride, groups=C // cpg)).contiguous()
    X.check_budget(ref, 9 * cpg, x, wt, bf16_out=True)
    assert X.small_share(ref) >= 0.9
    return _cl(x), _repack_w3_grouped(wt.cuda()), ref


def _assert_route(x, w3, stride, slices):
    """The non-split route folds BN stats, the split-K route cannot: the
    stats return tells which one the shape takes."""
    _, part = _e().conv3x3_fwd_stats(x, w3, stride)
    assert (part is not None) == (slices == 1)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape,stride,slices", DENSE)
def test_dense_bit_equal_to_conv_then_bn(shape, stride, slices, relu):
    e = _e()
    x, w3, ref = _dense_case(shape, stride)
    _assert_route(x, w3, stride, slices)
    n, ci, h, w, co = shape
    scale, shift = _affine(co, co + stride)
    xp = e.pad_nhwc(x)
    xp0, s0, t0 = xp.clone(), scale.clone(), shift.clone()
    for call in range(2):  # the second is wrong if the split-K pool is dirty
        got = e.conv3x3_fwd_bn_padded(xp, w3, stride, h, w, scale, shift, relu)
        want = e.bn_fwd_eval(e.conv3x3_fwd_padded(xp, w3, stride, h, w),
                             scale, shift, None, relu)
        assert got.dtype == torch.bfloat16 and got.shape == ref.shape
        assert torch.equal(got, want), call
    assert torch.equal(xp, xp0) and torch.equal(scale, s0) \
        and torch.equal(shift, t0)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("cpg,stride", GROUPED)
def test_grouped_bit_equal_to_conv_then_bn(cpg, stride, relu):
    e = _e()
    x, w3g, ref = _grouped_case(cpg, stride)
    co = x.shape[1]
    scale, shift = _affine(co, cpg + stride)
    got = e.conv3x3_grouped_fwd_bn(x, w3g, stride, scale, shift, relu)
    want = e.bn_fwd_eval(e.conv3x3_grouped_fwd(x, w3g, stride), scale, shift,
                         None, relu)
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape
    assert torch.equal(got, want)


def _check_bound(name, got, ref, scale, shift, relu):
    """Against fp64 relu?(yb*scale + shift), yb the exact conv rounded once
    to bf16; the bound is derived in affine_bound_ratio."""
    yb = ref.to(torch.bfloat16).double()
    ratio = affine_bound_ratio(got, yb, scale, shift, torch.zeros_like(yb),
                               relu)
    print(f"\nconv3x3 bn err/bound {name} relu={relu}: {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("shape,stride,slices", [DENSE[0], DENSE[2], DENSE[3]])
def test_dense_exact_reference(shape, stride, slices):
    """One independent check per route: 2 slices, 9 slices, non-split."""
    x, w3, ref = _dense_case(shape, stride)
    n, ci, h, w, co = shape
    scale, shift = _affine(co, 17 + co)
    xp = _e().pad_nhwc(x)
    for relu in (False, True):
        got = _e().conv3x3_fwd_bn_padded(xp, w3, stride, h, w, scale, shift,
                                         relu)
        _check_bound(f"{shape} s{stride} ({slices} slices)", got, ref, scale,
                     shift, relu)


@pytest.mark.parametrize("cpg", [16, 64])
def test_grouped_exact_reference(cpg):
    x, w3g, ref = _grouped_case(cpg, 1)
    scale, shift = _affine(x.shape[1], 23 + cpg)
    for relu in (False, True):
        got = _e().conv3x3_grouped_fwd_bn(x, w3g, 1, scale, shift, relu)
        _check_bound(f"grouped cpg{cpg}", got, ref, scale, shift, relu)


def test_refusals():
    e = _e()
    x, w3, _ = _dense_case(DENSE[0][0], 1)
    n, ci, h, w, co = DENSE[0][0]
    xp = e.pad_nhwc(x)
    scale, shift = _affine(co, 1)
    with pytest.raises(RuntimeError, match="fp32"):
        e.conv3x3_fwd_bn_padded(xp, w3, 1, h, w, scale.double(), shift, True)
    with pytest.raises(RuntimeError, match="shape"):
        e.conv3x3_fwd_bn_padded(xp, w3, 1, h, w, scale[:-1], shift, True)
    with pytest.raises(RuntimeError, match="device"):
        e.conv3x3_fwd_bn_padded(xp, w3, 1, h, w, scale, shift.cpu(), True)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.conv3x3_fwd_bn_padded(xp, w3, 1, h, w,
                                torch.cat([scale, scale])[::2], shift, True)
    xg, w3g, _ = _grouped_case(16, 1)
    sg, tg = _affine(xg.shape[1], 2)
    with pytest.raises(RuntimeError, match="shape"):
        e.conv3x3_grouped_fwd_bn(xg, w3g, 1, sg, torch.cat([tg, tg]), True)
    with pytest.raises(RuntimeError, match="fp32"):
        e.conv3x3_grouped_fwd_bn(xg, w3g, 1, sg.to(torch.bfloat16), tg, True)
