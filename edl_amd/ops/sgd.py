"""FusedSGD — momentum SGD over the reducer's flat buckets.

Replaces the reference's Paddle Momentum optimizer + fused-allreduce combo
(train_with_fleet.py:106-111 SGD momentum + L2 decay). Because
BucketedAllReducer re-homes both params and grads into flat per-bucket
buffers, the whole model update is ONE HIP kernel launch per bucket
(edl_amd._C.fused_sgd) instead of one per parameter tensor — and the DP
gradient average (1/world) is folded in as grad_scale, saving a full
read+write pass over all gradients.

State-dict format matches torch.optim.SGD (per-param momentum_buffer,
indexed in bucket order over the bucket params), so checkpoints survive
re-bucketing across elastic resizes."""
import torch

from . import available, ext
from .flat_optimizer import FlatBucketOptimizer


class FusedSGD(FlatBucketOptimizer):
    _name = "FusedSGD"
    _state_names = ("m",)
    _state_keys = {"momentum_buffer": "m"}
    _hyper_keys = ("lr", "momentum", "weight_decay")
    _bucket_order = True

    def __init__(self, params, lr=0.1, momentum=0.9, weight_decay=1e-4, grad_scale=1.0,
                 reducer=None):
        # params is accepted for API parity; the flat buffers come from the
        # reducer (set via attach() or inferred from param .grad views).
        super().__init__(
            params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay),
            grad_scale=grad_scale, reducer=reducer)
        self._use_ext = available() and torch.cuda.is_available()

    @torch.no_grad()
    def step(self, momentum=None, weight_decay=None, clip_state=None):
        """momentum / weight_decay override the group's values for this
        step only (None = the group's). DGC momentum correction steps
        with 0.0, 0.0: both already live in its accumulators, and with
        momentum 0 the momentum buffer just mirrors the update.
        clip_state: the [coef, norm, skip, nskipped] tensor of
        ops/clip.py GradClipper.run() — the gradient scale is multiplied
        by coef, and skip != 0 leaves p and m untouched."""
        from .conv import bump_weight_epoch

        bump_weight_epoch()  # invalidate per-step weight-derived caches
        g0 = self.param_groups[0]
        lr, mu, wd = g0["lr"], g0["momentum"], g0["weight_decay"]
        if momentum is not None:
            mu = float(momentum)
        if weight_decay is not None:
            wd = float(weight_decay)
        for bk in self._materialize():
            if self._use_ext and bk["p"].is_cuda:
                ext().fused_sgd(bk["p"], bk["g"], bk["m"], lr, mu, wd,
                                self.grad_scale, self._lr_dev, clip_state)
            else:
                # torch fallback (CPU tests / bring-up): same math
                g = self._cpu_grad(bk, clip_state)
                if g is None:
                    return  # skipped step: p, m untouched
                g = g.add(bk["p"], alpha=wd)
                bk["m"].mul_(mu).add_(g)
                bk["p"].add_(bk["m"], alpha=-lr)
