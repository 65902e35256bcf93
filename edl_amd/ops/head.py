"""The classifier head on CDNA4 kernels: global average pool + FC (parity:
the reference model zoo's pool2d(global) + fc tail,
example/distill/resnet/models/resnet_vd.py).

`pool_linear(x, fc)` computes `fc(avgpool(x).flatten(1))`. On a bf16
channels_last GPU tensor it runs csrc/head.hip: two launches forward (pool,
skinny MFMA GEMM with the fp32 bias in the epilogue), two backward (dx
broadcast over the pixels; dW and db in one launch, added straight into the
bucket-view gradients in direct-grad mode). The fp32 master weight is never
cast per step: the kernels read the engine's bf16 mirror view
(`weight._edl_bf16`) or a cast cached on the module. Everything else (CPU,
fp32, fp16, shapes outside the kernels' range, EDL_HEAD=0) takes the two
torch ops exactly as the models did before."""
import os

import torch
import torch.nn.functional as F

from . import available, ext
from . import conv as _conv

# 1: the HIP head where it applies; 0: adaptive_avg_pool2d + linear always
_HEAD = os.environ.get("EDL_HEAD", "1") != "0"

# the range head_fwd / head_bwd accept (csrc/launchers.h, module.cpp)
_MAX_ROWS = 512
_MAX_C = 4096
# Routing rule: the kernels walk the batch in passes of 64 rows and stream W
# again for every pass, which is right for the training and serving batches
# (16-32 rows: 1.2-1.8x over torch, tools/head_bench.py) and wrong for a wide
# one: at N = 256 the forward measured 102.6 us against torch's 30.3 us and
# forward+backward 265 us against 235 us (profiles/head_per_shape.txt). So
# pool_linear takes the HIP head for one pass only; wider batches stay on
# torch. 33-64 rows are one pass as well but were not timed.
_MAX_ROUTE_ROWS = 64


def _aligned(t):
    return t.data_ptr() % 16 == 0


def _in_range(x, fc):
    n, c, h, w = x.shape
    return (fc.in_features == c and c % 64 == 0 and 64 <= c <= _MAX_C
            and 1 <= n <= min(_MAX_ROWS, _MAX_ROUTE_ROWS) and h * w >= 1 and fc.out_features >= 1
            and n * h * w * c < 2 ** 31)


def _hip_route(x, fc):
    w = fc.weight
    return (_HEAD and x.is_cuda and x.dim() == 4
            and x.dtype == torch.bfloat16 and w.device == x.device
            and (w.dtype == torch.bfloat16
                 or (w.dtype == torch.float32
                     and torch.is_autocast_enabled()
                     and torch.get_autocast_dtype("cuda") == torch.bfloat16))
            and x.is_contiguous(memory_format=torch.channels_last)
            and _aligned(x) and _in_range(x, fc) and available())


def _weight_bf16(fc):
    """The [K, C] bf16 compute copy of fc.weight: the engine's mirror view
    when it has set one, the weight itself when it is bf16, else a cast
    cached on the module. A trainable weight is keyed on the optimizer's
    weight epoch (and its version, for optimizers that do not bump the
    epoch); a frozen one on its version, so a load_state_dict on a serving
    teacher is never answered from a stale cast."""
    w = fc.weight
    mb = getattr(w, "_edl_bf16", None)
    if (mb is not None and mb.shape == w.shape and mb.is_contiguous()
            and _aligned(mb)):
        return mb
    if w.dtype == torch.bfloat16 and w.is_contiguous() and _aligned(w):
        return w.detach()
    key = ((_conv._weight_epoch if w.requires_grad else -1), w._version,
           w.data_ptr())
    cache = getattr(fc, "_edl_head_w", None)
    if cache is None or cache[0] != key:
        cache = (key, w.detach().to(torch.bfloat16).contiguous())
        fc._edl_head_w = cache
    return cache[1]


def _direct_grad(p, training):
    """Conv2dFast._direct_grad for an fc parameter: the bucket-view fp32
    gradient the dW/db kernel adds into, or None."""
    if (p is not None and getattr(p, "_edl_direct_grad", False)
            and p.grad is not None and p.grad.dtype == torch.float32
            and p.grad.is_contiguous() and _aligned(p.grad)
            and torch.is_grad_enabled() and training):
        return p.grad
    return None


class _HeadFn(torch.autograd.Function):
    """Saves pooled [N, C], never x."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_bf16, dw_tgt, db_tgt):
        b32 = None
        if bias is not None:
            b32 = bias.detach()
            if b32.dtype != torch.float32 or not _aligned(b32):
                b32 = b32.float().clone()
        logits, pooled = ext().head_fwd(x, w_bf16, b32)
        ctx.save_for_backward(pooled)
        ctx.w_bf16 = w_bf16
        ctx.hw = (x.shape[2], x.shape[3])
        ctx.tgt = (dw_tgt, db_tgt)
        ctx.dtypes = (weight.dtype, None if bias is None else bias.dtype)
        return logits

    @staticmethod
    def backward(ctx, dl):
        (pooled,) = ctx.saved_tensors
        dw_tgt, db_tgt = ctx.tgt
        dl = dl.to(torch.bfloat16).contiguous()
        if not _aligned(dl):
            dl = dl.clone()
        dx, dw, db = ext().head_bwd(dl, pooled, ctx.w_bf16, ctx.hw[0],
                                    ctx.hw[1], ctx.needs_input_grad[0],
                                    dw_tgt, db_tgt)
        wdt, bdt = ctx.dtypes
        if dw is not None:
            dw = dw.to(wdt) if ctx.needs_input_grad[1] else None
        if db is not None:
            db = db.to(bdt) if bdt is not None and ctx.needs_input_grad[2] \
                else None
        return dx, dw, db, None, None, None


def pool_linear(x, fc):
    """fc(adaptive_avg_pool2d(x, 1).flatten(1)) for an nn.Linear `fc`."""
    if not _hip_route(x, fc):
        return fc(F.adaptive_avg_pool2d(x, 1).flatten(1))
    w_bf16 = _weight_bf16(fc)
    if not (torch.is_grad_enabled()
            and (x.requires_grad or fc.weight.requires_grad
                 or (fc.bias is not None and fc.bias.requires_grad))):
        # teacher serving, evaluate(): forward only
        b32 = fc.bias
        if b32 is not None and (b32.dtype != torch.float32
                                or not _aligned(b32)):
            b32 = b32.float().clone()
        return ext().head_fwd(x, w_bf16, b32)[0]
    dw_tgt = _direct_grad(fc.weight, fc.training)
    db_tgt = _direct_grad(fc.bias, fc.training)
    return _HeadFn.apply(x, fc.weight, fc.bias, w_bf16, dw_tgt, db_tgt)
