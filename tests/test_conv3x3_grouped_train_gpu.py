"""Grouped 3x3 conv backward (conv3x3.hip GROUPED dgrad, gemm_tn.hip GRP
wgrad, ops/conv.py _Conv3x3GroupedHip) against fp64 CPU references, bit for
bit on integer operands (tests/_mfma_exact_common.py), plus one real-valued
wgrad under the derived accumulation bound.

Every (cpg, C) has two 64-wide tiles, so the channel-window base is
exercised; (128, 256) has two n-tiles inside one group. The geometries span
an image boundary, give parity classes of unequal size, and make M = 126 (a
full K chunk + a 62-row tail) at stride 1 and M = 40 (one partial chunk) at
stride 2.
"""
import functools

import pytest
import torch

import _mfma_exact_common as X

pytestmark = pytest.mark.gpu

CPG_C = [(16, 128), (32, 128), (64, 128), (128, 256)]
GEOM = [(1, 7, 9), (2, 7, 9), (2, 8, 10)]  # stride, H, W; N = 2


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e():
    from edl_amd import ops
    return ops.ext()


def _ref_dx(x_shape, w, dy, stride, groups):
    return torch.nn.grad.conv2d_input(
        list(x_shape), X._d(w), X._d(dy).contiguous(), stride=stride,
        padding=1, groups=groups)


def _ref_dw(x, w_shape, dy, stride, groups):
    return torch.nn.grad.conv2d_weight(
        X._d(x).contiguous(), tuple(w_shape), X._d(dy).contiguous(),
        stride=stride, padding=1, groups=groups)


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(cpg, C, stride, H, W):
    """CPU operands and both references, budgets asserted on the
    references before any kernel output is looked at."""
    gen = torch.Generator().manual_seed(7 * cpg + C + 100 * stride + H)
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = X.ints((2, C, H, W), X.PM12, gen)
    w = X.ints((C, cpg, 3, 3), X.ASYM3, gen)
    dy = X.ints((2, C, ho, wo), X.PM1, gen)
    dx = _ref_dx(x.shape, w, dy, stride, C // cpg)
    dw = _ref_dw(x, w.shape, dy, stride, C // cpg)
    X.check_budget(dx, 9 * cpg, dy, w, bf16_out=True)
    X.check_budget(dw, 2 * ho * wo, dy, x, bf16_out=False)
    return x, w, dy, dx, dw


def _wgrad(x, dy, stride, cpg, splitk):
    e = _e()
    return e.gemm_tn3x3_grouped_splitk_padded(
        X.rows(dy).contiguous().cuda(), e.pad_nhwc(_cl(x)), x.shape[2],
        x.shape[3], stride, max(cpg, 64), splitk)


def _check_wgrad(dw3g, dw_ref, cpg, what):
    from edl_amd.ops.conv import _unpack_dw3_grouped
    C = dw_ref.shape[0]
    if cpg >= 64:  # the raw layout IS [C, 9*gw] s-major
        X.check_exact(dw3g, dw_ref.permute(0, 2, 3, 1).reshape(C, -1), what)
    X.check_exact(_unpack_dw3_grouped(dw3g, cpg).contiguous(), dw_ref, what)


# + M = 392 (six full chunks and a tail, more than one split-K slice)
@pytest.mark.parametrize("cpg,C,stride,H,W,splitk", [
    (cpg, C, s, H, W, 0) for cpg, C in CPG_C for s, H, W in GEOM] + [
    (cpg, C, 1, 14, 14, sk) for cpg, C in (CPG_C[0], CPG_C[3])
    for sk in (0, 3)])
def test_grouped_wgrad_exact(cpg, C, stride, H, W, splitk):
    x, _, dy, _, dw = _case(cpg, C, stride, H, W)
    _check_wgrad(_wgrad(x, dy, stride, cpg, splitk), dw, cpg,
                 f"wgrad cpg{cpg} s{stride} {H}x{W} splitk{splitk}")


@pytest.mark.parametrize("stride,H,W", GEOM)
@pytest.mark.parametrize("cpg,C", CPG_C)
def test_grouped_dgrad_exact(cpg, C, stride, H, W):
    from edl_amd.ops import conv as cv
    x, w, dy, dx, _ = _case(cpg, C, stride, H, W)
    if stride == 1:
        got = _e().conv3x3_grouped_fwd(
            _cl(dy), cv._repack_w3_grouped_rot(w.cuda()), 1)
    else:
        got = _e().conv3x3s2_dgrad_grouped(
            _cl(dy), cv._repack_w3_s2dgrad_grouped(w.cuda()), H, W)
    X.check_exact(got, X.rows(dx), f"dgrad cpg{cpg} s{stride} {H}x{W}")


@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("stride,H,W", GEOM[:2])
@pytest.mark.parametrize("cpg,C", [(16, 128), (64, 128)])
def test_grouped_module_backward(monkeypatch, cpg, C, stride, H, W, train):
    from edl_amd.ops import conv as cv
    x, w, dy, dx, dw = _case(cpg, C, stride, H, W)
    e, calls = _e(), {}
    dgrad = "conv3x3_grouped_fwd" if stride == 1 else "conv3x3s2_dgrad_grouped"
    names = ("conv3x3_grouped_fwd_padded", dgrad,
             "gemm_tn3x3_grouped_splitk_padded")

    def counted(name, fn):
        def f(*a):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a)
        return f

    for name in names:
        monkeypatch.setattr(e, name, counted(name, getattr(e, name)))
    monkeypatch.setattr(cv, "_GROUPED_TRAIN", bool(train))
    m = cv.Conv2dFast(C, C, 3, stride, 1, groups=C // cpg, bias=False)
    m = m.cuda().to(torch.bfloat16)
    with torch.no_grad():
        m.weight.copy_(w)
    xg = _cl(x).requires_grad_(True)
    m(xg).backward(_cl(dy))
    if not train:  # the library route: gradients arrive, no new binding runs
        assert calls == {} and xg.grad is not None and m.weight.grad is not None
        return
    assert calls == dict.fromkeys(names, 1), calls
    X.check_exact(xg.grad, dx, "module x.grad")
    X.check_exact(m.weight.grad, dw, "module weight.grad")


def test_grouped_wgrad_real_bound():
    """randn operands, cpg 64, M = 392: rounding inside the accumulator,
    which integers cannot show. Measured max(err/bound) on an MI355X:
    see docs/kernels.md (grouped 3x3 backward)."""
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 128, 14, 14, generator=gen).to(torch.bfloat16)
    dy = torch.randn(2, 128, 14, 14, generator=gen).to(torch.bfloat16)
    ref = _ref_dw(x, (128, 64, 3, 3), dy, 1, 2)
    absprod = _ref_dw(x.abs(), (128, 64, 3, 3), dy.abs(), 1, 2)
    from edl_amd.ops.conv import _unpack_dw3_grouped
    got = _unpack_dw3_grouped(_wgrad(x, dy, 1, 64, 0), 64)
    ratio = X.bound_ratio(got, ref, absprod, 392)
    print("grouped wgrad real-valued max(err/bound) = %.4f" % ratio)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("bad", ["gw", "dtype", "extent"])
@pytest.mark.parametrize("which", ["wgrad", "dgrad"])
def test_grouped_bindings_refuse(which, bad):
    e = _e()
    C = 192 if bad == "gw" else 128        # gw 128 does not divide 192
    dy = torch.ones(1, C, 4, 4, device="cuda", dtype=torch.bfloat16)
    dy = dy.contiguous(memory_format=torch.channels_last)
    if bad == "dtype":
        dy = dy.float()
    H = 9 if bad == "extent" else 8        # dy is 4x4: an 8x8 image, stride 2
    with pytest.raises(RuntimeError):
        if which == "wgrad":
            xp = torch.zeros(1, 10, 10, C, device="cuda", dtype=torch.bfloat16)
            e.gemm_tn3x3_grouped_splitk_padded(
                X.rows(dy).contiguous(), xp, H, 8, 2, 128, 0)
        else:
            wcat = torch.zeros(C, 9 * 128, device="cuda", dtype=torch.bfloat16)
            e.conv3x3s2_dgrad_grouped(dy, wcat, H, 8)
