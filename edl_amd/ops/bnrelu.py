"""Fused BatchNorm(+Add)+ReLU modules backed by the CDNA4 kernels.

BNReLU2d / BNAddReLU2d replace (BatchNorm2d, ReLU) and the bottleneck tail
(BatchNorm2d, +residual, ReLU). On GPU with bf16 channels_last input the
HIP kernels run (fp32 math, no autocast cast traffic, no
num_batches_tracked kernel); anywhere else a plain torch reference runs —
the same math the numerics tests compare against.

State-dict layout matches nn.BatchNorm2d (weight/bias/running_mean/
running_var/num_batches_tracked), so checkpoints interchange."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import available, ext
from . import conv as _conv
from .conv import padded_interior


def _direct_grad(p):
    """Direct-grad mode (reducer sets _edl_direct_grad at world 1): the
    param's bucket-view gradient to accumulate into in-kernel, or None."""
    if (getattr(p, "_edl_direct_grad", False) and p.grad is not None
            and p.grad.dtype == torch.float32 and p.grad.is_contiguous()):
        return p.grad
    return None


class _FusedBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, rmean, rvar, momentum, eps, res2d, relu,
                pre_part=None, pad_out=None, dx_pad=None):
        # x: the [M, C] view, or the 4-D channels_last tensor itself (then
        # y comes back 4-D too). The two padded-layout hand-offs to a 3x3
        # conv (conv.py) need the 4-D form on their side, because the
        # interior of a padded buffer is no [M, C] view:
        #  pad_out (list): y is written into the zero-halo padded buffer,
        #    which is appended to the list; the [N, C, H, W] interior view
        #    is returned. Needs relu, no residual.
        #  dx_pad (list, 4-D x only): backward writes dx padded, leaves
        #    the buffer in the list (the producing conv's backward pops
        #    it) and returns the interior view as the gradient.
        ctx.shape4 = tuple(x.shape) if x.dim() == 4 else None
        x2d = _to_2d(x) if x.dim() == 4 else x
        assert ctx.shape4 is not None or (pad_out is None and dx_pad is None)
        y, mean, invstd, mask = ext().bn_fwd_train(
            x2d, gamma, beta, rmean, rvar, momentum, eps, res2d, relu,
            pre_part, ctx.shape4[2:] if pad_out is not None else None
        )
        # backward reads the 1-bit ReLU mask instead of y (16x fewer bytes)
        ctx.save_for_backward(x2d, mask, mean, invstd, gamma)
        ctx.relu = relu
        ctx.has_res = res2d is not None
        ctx.dg_t = _direct_grad(gamma)
        ctx.db_t = _direct_grad(beta)
        ctx.dx_pad = dx_pad
        if pad_out is not None:
            pad_out.append(y)
            return padded_interior(y)
        return _from_2d(y, ctx.shape4) if ctx.shape4 is not None else y

    @staticmethod
    def backward(ctx, dy):
        x2d, mask, mean, invstd, gamma = ctx.saved_tensors
        if dy.dim() == 4:
            dy = _to_2d(dy)
        dx, dgamma, dbeta, dres = ext().bn_bwd(
            dy, mask, x2d, mean, invstd, gamma, ctx.relu, ctx.has_res, True,
            ctx.dg_t, ctx.db_t,
            ctx.shape4[2:] if ctx.dx_pad is not None else None
        )
        if dx.dim() == 4:  # padded [N, H+2, W+2, C]
            ctx.dx_pad[:] = [dx]
            dx = padded_interior(dx)
        elif ctx.shape4 is not None:
            dx = _from_2d(dx, ctx.shape4)
        return (dx,
                None if ctx.dg_t is not None else dgamma,
                None if ctx.db_t is not None else dbeta,
                None, None, None, None,
                dres if ctx.has_res else None, None, None, None, None)


def _to_2d(t):
    """NCHW-channels_last tensor -> [M, C] contiguous view (zero-copy)."""
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c)


def _from_2d(t2d, shape):
    n, c, h, w = shape
    return t2d.view(n, h, w, c).permute(0, 3, 1, 2)


class BNReLU2d(nn.Module):
    """BatchNorm2d (+ optional fused ReLU). act=False gives plain BN."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, act=True):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.act = act
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        # batch count kept as a host int (no per-step device kernel like
        # nn.BatchNorm2d's add_); synced into the buffer at state_dict time
        # so checkpoints carry the real count (momentum=None consumers need
        # it for cumulative averaging). Steps replayed inside a captured
        # hipGraph don't re-run forward and are not counted.
        self._batches_seen = 0
        self.register_state_dict_pre_hook(type(self)._sync_batches_to_buffer)
        self.register_load_state_dict_post_hook(type(self)._sync_batches_from_buffer)

    def _sync_batches_to_buffer(self, *args, **kwargs):
        self.num_batches_tracked.fill_(self._batches_seen)

    def _sync_batches_from_buffer(self, *args, **kwargs):
        self._batches_seen = int(self.num_batches_tracked.item())

    def _use_fused(self, x, res=None):
        if not (x.is_cuda and x.dtype == torch.bfloat16 and available()):
            return False
        if not x.is_contiguous(memory_format=torch.channels_last):
            return False
        return self._fused_applies(res)

    def _fused_applies(self, res=None):
        """The part of _use_fused that does not look at x: what the module,
        the mode and the residual allow for a bf16 channels_last GPU input
        (ops.conv.conv_bn asks before the conv output exists)."""
        import os

        if os.environ.get("EDL_FUSED_BN", "1") != "1":
            return False
        if self.num_features % 8 != 0:
            return False
        wide = self.num_features > 2048
        if wide or self.num_features & (self.num_features - 1):
            # training reduce kernels cap at 2048 (LDS) and need a pow2
            # width (row partition); the EVAL apply kernel has neither
            # limit — wide teachers opt in until the round-3 GPU
            # validation (EDL_BN_WIDE_EVAL=1; see NOTES r2c42)
            if (self.training or torch.is_grad_enabled() or
                    (wide and os.environ.get("EDL_BN_WIDE_EVAL", "0") != "1")):
                return False
        if res is not None and (
            res.dtype != torch.bfloat16
            or not res.is_contiguous(memory_format=torch.channels_last)
        ):
            return False
        return True

    def _fallback(self, x, res=None):
        y = F.batch_norm(
            x.float(), self.running_mean, self.running_var, self.weight, self.bias,
            self.training, self.momentum, self.eps,
        )
        if res is not None:
            y = y + res.float()
        if self.act:
            y = F.relu(y)
        return y.to(x.dtype)

    def _fused(self, x, res=None, partials=None, pad_out=False, dx_pad=None):
        x2d = _to_2d(x)
        res2d = _to_2d(res) if res is not None else None
        if self.training:
            # padded-layout hand-offs to a neighbouring 3x3 conv (see
            # _FusedBN.forward); both are plain-BN(+ReLU) only
            pad_out = (pad_out and self.act and res is None
                       and _conv._PAD_ONCE and _conv._BN_PAD_OUT)
            if res is not None or not (_conv._PAD_ONCE and _conv._BN_PAD_DX):
                dx_pad = None
            if pad_out or dx_pad is not None:
                holder = [] if pad_out else None
                y = _FusedBN.apply(
                    x, self.weight, self.bias, self.running_mean,
                    self.running_var, self.momentum, self.eps, None, self.act,
                    partials, holder, dx_pad,
                )
                if pad_out:
                    # the consumer (Conv2dFast) finds the padded buffer here
                    y._edl_xp = holder[0]
                return y
            y2d = _FusedBN.apply(
                x2d, self.weight, self.bias, self.running_mean, self.running_var,
                self.momentum, self.eps, res2d, self.act, partials,
            )
        else:
            scale, shift = self.eval_scale_shift()
            y2d = ext().bn_fwd_eval(x2d, scale, shift, res2d, self.act)
        return _from_2d(y2d, x.shape)

    def eval_scale_shift(self):
        """(scale, shift), fp32 [C]: the eval-mode BN as y = x*scale + shift.

        They depend only on (weight, bias, running stats) and are cached,
        keyed on the four tensors' device, data_ptr() and in-place versions
        (a .to() or a replaced parameter gives fresh tensors whose versions
        restart, so the versions alone can collide). Recomputing per forward
        cost ~4 tiny kernels x ~104 BN layers per ResNeXt101 teacher fwd
        (~300 ms/s of pure launch + elementwise overhead in the distill
        teacher trace r2c41). The key does NOT see kernel writes
        (bn_fwd_train, fused_sgd, graph replay go through raw pointers):
        TrainerEngine.evaluate() invalidates _eval_ver explicitly."""
        ver = tuple((t.device, t.data_ptr(), t._version)
                    for t in (self.weight, self.bias, self.running_mean,
                              self.running_var))
        if getattr(self, "_eval_ver", None) != ver:
            invstd = torch.rsqrt(self.running_var + self.eps)
            scale = self.weight * invstd
            self._eval_scale = scale
            self._eval_shift = self.bias - self.running_mean * scale
            self._eval_ver = ver
        return self._eval_scale, self._eval_shift

    def forward(self, x, res=None, partials=None, pad_out=False, dx_pad=None):
        # partials: BN stats pre-folded into the producing conv's
        # epilogue ([tiles, 2C] fp32) — skips the stats kernel.
        # pad_out: the output feeds exactly one padded-input 3x3 conv —
        # write it in the padded layout (returned tensor carries _edl_xp).
        # dx_pad: the producing conv's pop_dy_pad() holder.
        # Both are honoured on the fused training path only; everywhere
        # else the conv pads for itself.
        if self.training:
            self._batches_seen += 1
        if self._use_fused(x, res):
            if self.training or not torch.is_grad_enabled():
                return self._fused(x, res,
                                   partials if self.training else None,
                                   pad_out, dx_pad)
        if partials is not None:
            # capped partials come from a pooled buffer that the finalize
            # kernel normally returns clean; if we're not consuming them,
            # scrub before dropping so the pool stays zeroed
            partials.zero_()
        return self._fallback(x, res)

    def extra_repr(self):
        return "%d, act=%s" % (self.num_features, self.act)


class BNAddReLU2d(BNReLU2d):
    """The bottleneck tail: relu(bn(x) + residual) as one fused op."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__(num_features, eps=eps, momentum=momentum, act=True)

    def forward(self, x, res, partials=None):  # res is mandatory here
        return super().forward(x, res, partials)
