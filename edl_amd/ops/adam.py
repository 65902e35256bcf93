"""FusedAdam / FusedAdamW — Adam over the reducer's flat buckets.

The reference trains its CTR, fit_a_line and recognize_digits models with
Adam (example/ctr/ctr/train.py:234), its NLP distillation students with
AdamW minus decay on biases and norm scales (example/distill/nlp/
model.py:35-51), and its ResNet script has an `adam` strategy
(train_with_fleet.py:196-200). Like FusedSGD, the whole model update is ONE
HIP launch per bucket (edl_amd._C.fused_adam) with the DP gradient average
and the fp16 loss-scale inverse folded in as grad_scale.

Semantics are torch.optim.Adam / AdamW (no amsgrad, no maximize). What
changes between steps lives on the device: the LR scalar and the int32
step counter, which step() advances with a captured op and the kernel turns
into bias corrections itself — so a hipGraph-captured step keeps counting
on replay, where no host code runs. On GPU that counter is the source of
truth (state_dict() reads it back); on CPU the same tensor lives on the
host and the update is the torch op sequence of torch.optim.Adam.

no_decay (None | predicate param -> bool | iterable of params) exempts
params from weight decay. Adjacent params of a bucket with equal decay
coalesce into one segment of the kernel's decay table; a bucket whose
params all agree needs no table. The kernel takes at most MAX_SEGMENTS
(1024) segments per bucket.

State-dict format matches torch.optim.Adam (per-param step / exp_avg /
exp_avg_sq, indexed in the order the params were given), so checkpoints
interchange with torch and survive re-bucketing across elastic resizes."""
import torch

from . import ext
from .flat_optimizer import MAX_SEGMENTS, FlatBucketOptimizer

ADAM_MAX_SEGMENTS = MAX_SEGMENTS


class FusedAdam(FlatBucketOptimizer):
    _name = "FusedAdam"
    _state_names = ("m", "v")
    _state_keys = {"exp_avg": "m", "exp_avg_sq": "v"}
    _hyper_keys = ("lr", "eps", "weight_decay", "betas")
    _select_key = "no_decay"
    _table_kind = "decay"
    _cap_message = ("a bucket alternates decay %d times; the kernel's table "
                    "holds %d segments per bucket (use a smaller bucket cap)")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, decoupled=False, no_decay=None,
                 grad_scale=1.0, reducer=None):
        betas = (float(betas[0]), float(betas[1]))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdam: betas must lie in [0, 1)")
        if eps < 0.0 or lr < 0.0 or weight_decay < 0.0:
            raise ValueError("FusedAdam: lr, eps, weight_decay must be >= 0")
        # int32 [1] on the buckets' device: THE step count (see module doc)
        self._step_t = None
        super().__init__(
            params,
            dict(lr=float(lr), betas=betas, eps=float(eps),
                 weight_decay=float(weight_decay), amsgrad=False,
                 decoupled=bool(decoupled)),
            select=no_decay, grad_scale=grad_scale, reducer=reducer)

    @property
    def step_count(self):
        """Optimizer steps taken (reads the device counter back on GPU)."""
        return 0 if self._step_t is None else int(self._step_t.item())

    def _build_tables(self):
        """Per bucket: coalesce adjacent params of equal decay into
        segments; one segment = uniform decay, no table."""
        for bk in self._buckets:
            self._build_segments(bk, merge=lambda prev, wd: prev == wd)
            segs = bk["segs"]
            bk["wd"] = segs[0][1] if len(segs) == 1 else 0.0

    def _on_materialize(self, buckets):
        self._build_tables()
        if buckets and self._step_t is None:  # survives rebuild(): m, v do not
            self._step_t = torch.zeros(1, dtype=torch.int32,
                                       device=buckets[0]["p"].device)

    @torch.no_grad()
    def step(self, clip_state=None):
        """clip_state: the [coef, norm, skip, nskipped] tensor of
        ops/clip.py GradClipper.run() — the gradient scale is multiplied
        by coef; skip != 0 leaves p, m, v AND the step count untouched."""
        from .conv import bump_weight_epoch

        bump_weight_epoch()  # invalidate per-step weight-derived caches
        buckets = self._materialize()
        if not buckets:
            return
        g0 = self.param_groups[0]
        lr, (b1, b2), eps = g0["lr"], g0["betas"], g0["eps"]
        decoupled = g0["decoupled"]
        # once per step for all buckets; an in-place device op, so a graph
        # capture records it and every replay counts. With a clip state the
        # counter advances by 1 - skip, still on the device.
        if clip_state is None:
            self._step_t.add_(1)
        else:
            self._step_t.add_((1.0 - clip_state[2:3]).to(torch.int32))
        if buckets[0]["p"].is_cuda:
            fused_adam = ext().fused_adam  # a missing kernel is an error
            for bk in buckets:
                fused_adam(bk["p"], bk["g"], bk["m"], bk["v"], self._step_t,
                           lr, b1, b2, eps, bk["wd"], self.grad_scale,
                           decoupled, self._lr_dev, bk["seg_end"],
                           bk["seg_wd"], clip_state)
            return
        # CPU (tests / bring-up): torch.optim.Adam's own op sequence, with
        # the host step count authoritative
        if clip_state is not None and bool(clip_state[2] != 0):
            return  # skipped step
        t = int(self._step_t.item())
        bc1 = 1 - b1 ** t
        bc2 = 1 - b2 ** t
        step_size = lr / bc1
        bc2_sqrt = bc2 ** 0.5
        for bk in buckets:
            p, m, v = bk["p"], bk["m"], bk["v"]
            g = self._cpu_grad(bk, clip_state)
            start = 0
            for end, wd in bk["segs"]:
                if wd != 0.0:
                    if decoupled:
                        p[start:end].mul_(1 - lr * wd)
                    else:
                        if g is bk["g"]:
                            g = g.clone()
                        g[start:end].add_(p[start:end], alpha=wd)
                start = end
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (v.sqrt() / bc2_sqrt).add_(eps)
            p.addcdiv_(m, denom, value=-step_size)

    def state_buffers(self):
        """m, v per bucket and the step counter."""
        out = super().state_buffers()
        if self._step_t is not None:
            out.append(self._step_t)
        return out

    # ---- torch.optim.Adam-compatible state dict ----
    def _state_entry(self):
        return {"step": torch.tensor(float(self.step_count),
                                     dtype=torch.float32)}

    def load_state_dict(self, sd):
        """The moments, the step, lr, betas, eps and weight_decay are taken
        from `sd`. The decay MODE (`decoupled`, the `no_decay` set) is this
        optimizer's construction-time choice: a state dict that records
        another one (torch's own records neither) is refused with a
        ValueError before anything is loaded."""
        src = sd["param_groups"][0] if sd.get("param_groups") else {}
        mine = self.param_groups[0]["decoupled"]
        if "decoupled" in src and bool(src["decoupled"]) != mine:
            raise ValueError(
                "FusedAdam: state dict was saved with decoupled=%s, this "
                "optimizer has decoupled=%s" % (bool(src["decoupled"]), mine))
        super().load_state_dict(sd)

    def _on_load(self, entries, changed):
        steps = [int(float(e["step"])) for e in entries
                 if e.get("step") is not None]
        if steps and self._step_t is not None:
            # one shared counter: every param steps together here
            self._step_t.fill_(max(steps))
        if changed is not None:
            self._build_tables()  # weight_decay may have changed


class FusedAdamW(FusedAdam):
    """FusedAdam with decoupled weight decay (torch.optim.AdamW)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, no_decay=None, grad_scale=1.0,
                 reducer=None, decoupled=True):
        super().__init__(params, lr=lr, betas=betas, eps=eps,
                         weight_decay=weight_decay, decoupled=decoupled,
                         no_decay=no_decay, grad_scale=grad_scale,
                         reducer=reducer)
