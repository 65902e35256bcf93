"""Shared by the tests of the eval BN(+Add)+ReLU epilogues (gemm_bt_bn, the
conv3x3 *_bn bindings): the per-channel operands and the derived bound of
the independent fp64 check."""
import torch


def affine(n, g):
    """Per-channel scale/shift no two channels share: randn, with zero and
    negative scales and one channel of large shift."""
    scale = torch.randn(n, device="cuda", generator=g)
    shift = torch.randn(n, device="cuda", generator=g)
    scale[::7] = 0.0
    scale[1] = -1.5
    scale[n - 1] = -0.25
    shift[n // 2] = 1000.0
    return scale, shift


def affine_bound_ratio(got, yb64, scale, shift, r64, relu):
    """max(err / bound) of a fused output against the fp64 reference
    relu?(yb*scale + shift + r), yb the conv/GEMM result rounded once to
    bf16. Per element
        |got - ref| <= 2^-8 |ref| + 2^-22 (|yb*scale| + |shift| + |r|):
    one fp32 fma rounding and one fp32 add rounding (each at most 2^-24 of
    a value the sum in the second term bounds; taken twice), and the bf16
    rounding of the result v, half an ulp: at most 2^-8 |v| just above a
    power of two, with |v| within the second term of |ref|. ReLU is
    1-Lipschitz, so it widens nothing."""
    s, t = scale.double().cpu(), shift.double().cpu()
    pre = yb64 * s + t + r64
    ref = pre.clamp(min=0) if relu else pre
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * (
        (yb64 * s).abs() + t.abs() + r64.abs())
    err = (got.detach().cpu().double() - ref).abs()
    ok = bound > 0
    assert bool((err[~ok] == 0).all())  # bound 0: scale, shift, r all zero
    return (err[ok] / bound[ok]).max().item()
