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
host and the update is the torch op sequence of torch.optim.Adam. Buckets
on a GPU ALWAYS take the kernel: without the built extension step() raises
(ops.ext()) instead of running the torch math there — unlike FusedSGD's
`_use_ext` switch, on purpose: a missing kernel is an error in this
project, not a slower path taken quietly.

no_decay (None | predicate param -> bool | iterable of params) exempts
params from weight decay. Adjacent params of a bucket with equal decay
coalesce into one segment of the kernel's decay table; a bucket whose
params all agree needs no table. The kernel takes at most
ADAM_MAX_SEGMENTS (1024) segments per bucket.

State-dict format matches torch.optim.Adam (per-param step / exp_avg /
exp_avg_sq, indexed in the order the params were given), so checkpoints
interchange with torch and survive re-bucketing across elastic resizes."""
import torch

from . import ext
from ..train.bucketed_ddp import _view_like

ADAM_MAX_SEGMENTS = 1024  # == _C.ADAM_MAX_SEGMENTS (csrc/launchers.h)


class FusedAdam:
    handles_grad_scale = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, decoupled=False, no_decay=None,
                 grad_scale=1.0, reducer=None):
        betas = (float(betas[0]), float(betas[1]))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdam: betas must lie in [0, 1)")
        if eps < 0.0 or lr < 0.0 or weight_decay < 0.0:
            raise ValueError("FusedAdam: lr, eps, weight_decay must be >= 0")
        # state-dict indices follow the order given, as torch.optim does
        self._all_params = list(params)
        self._index = {id(p): i for i, p in enumerate(self._all_params)}
        if no_decay is None:
            nd = []
        elif callable(no_decay):
            nd = [i for i, p in enumerate(self._all_params) if no_decay(p)]
        else:
            ids = {id(p) for p in no_decay}
            nd = [i for i, p in enumerate(self._all_params) if id(p) in ids]
        self._no_decay = set(nd)
        self.defaults = dict(lr=float(lr), betas=betas, eps=float(eps),
                             weight_decay=float(weight_decay), amsgrad=False,
                             decoupled=bool(decoupled), no_decay=sorted(nd))
        self.param_groups = [dict(
            self.defaults,
            params=[p for p in self._all_params if p.requires_grad])]
        self.grad_scale = grad_scale
        self._reducer = reducer
        self._buckets = None
        # int32 [1] on the buckets' device: THE step count (see module doc)
        self._step_t = None
        # LR device scalar on GPU, read by the kernel at run time so a
        # captured step tracks set_lr() on replay
        self._lr_dev = None
        if reducer is not None:
            self.attach(reducer)

    def attach(self, reducer):
        self._reducer = reducer
        self._buckets = None
        reducer._attached_opt = self  # rebuild() snapshots/restores m, v, step
        return self

    def set_lr(self, lr):
        """Set the learning rate (updates the device scalar when present)."""
        for g in self.param_groups:
            g["lr"] = float(lr)
        if self._lr_dev is not None:
            self._lr_dev.fill_(float(lr))

    @property
    def step_count(self):
        """Optimizer steps taken (reads the device counter back on GPU)."""
        return 0 if self._step_t is None else int(self._step_t.item())

    def _param_wd(self, p):
        wd = self.param_groups[0]["weight_decay"]
        return 0.0 if self._index.get(id(p)) in self._no_decay else wd

    def _build_tables(self):
        """Per bucket: coalesce adjacent params of equal decay into
        segments; one segment = uniform decay, no table."""
        for bk in self._buckets:
            segs = []  # [end, wd]
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                wd = self._param_wd(p)
                if segs and segs[-1][1] == wd:
                    segs[-1][0] = off + n
                else:
                    segs.append([off + n, wd])
            bk["segs"] = segs
            bk["wd"] = segs[0][1] if len(segs) == 1 else 0.0
            bk["seg_end"] = bk["seg_wd"] = None
            if len(segs) > 1 and bk["p"].is_cuda:
                if len(segs) > ADAM_MAX_SEGMENTS:
                    raise RuntimeError(
                        "FusedAdam: a bucket alternates decay %d times; the "
                        "kernel's table holds %d segments per bucket (use a "
                        "smaller bucket cap)" % (len(segs), ADAM_MAX_SEGMENTS))
                # checked HERE, on the host lists: the binding can only
                # check a device table with a D2H sync, which it cannot
                # afford under graph capture
                ends = [s[0] for s in segs]
                if (ends != sorted(ends) or ends[-1] != bk["p"].numel()
                        or bk["p"].numel() >= 2 ** 31):
                    raise RuntimeError("FusedAdam: malformed decay table")
                dev = bk["p"].device
                bk["seg_end"] = torch.tensor([s[0] for s in segs],
                                             dtype=torch.int32, device=dev)
                bk["seg_wd"] = torch.tensor([s[1] for s in segs],
                                            dtype=torch.float32, device=dev)

    def _materialize(self):
        if self._buckets is not None:
            return self._buckets
        r = self._reducer
        if r is None:
            raise RuntimeError("FusedAdam needs a BucketedAllReducer (call attach())")
        out = []
        for b in r._buckets:
            if b.param_flat is None:
                raise RuntimeError("FusedAdam requires flatten_params=True buckets")
            offsets = []
            off = 0
            for p in b.params:
                offsets.append((off, p.numel()))
                off += p.numel()
            out.append({"p": b.param_flat, "g": b.buffer,
                        "m": torch.zeros_like(b.param_flat),
                        "v": torch.zeros_like(b.param_flat),
                        "params": b.params, "offsets": offsets})
        self._buckets = out
        self._build_tables()
        if out:
            dev = out[0]["p"].device
            if self._step_t is None:  # survives rebuild(): m, v do not
                self._step_t = torch.zeros(1, dtype=torch.int32, device=dev)
            if dev.type == "cuda" and self._lr_dev is None:
                self._lr_dev = torch.full(
                    (1,), self.param_groups[0]["lr"], dtype=torch.float32,
                    device=dev)
        return out

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
            g = bk["g"]
            if clip_state is not None:
                # fp32 product first, as the kernel forms it
                g = g.mul(clip_state[0] * self.grad_scale)
            elif self.grad_scale != 1.0:
                g = g.mul(self.grad_scale)
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

    def zero_grad(self, set_to_none=False):
        if self._reducer is not None:
            self._reducer.zero_grad()

    def state_buffers(self):
        """Every tensor that must agree across ranks: m, v per bucket and
        the step counter (the engine broadcasts them from rank 0)."""
        out = []
        for bk in self._materialize():
            out += [bk["m"], bk["v"]]
        if self._step_t is not None:
            out.append(self._step_t)
        return out

    # ---- torch.optim.Adam-compatible state dict ----
    def state_dict(self):
        state = {}
        buckets = self._materialize()
        t = float(self.step_count)
        for bk in buckets:
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                state[self._index[id(p)]] = {
                    "step": torch.tensor(t, dtype=torch.float32),
                    "exp_avg": _view_like(bk["m"][off:off + n], p).clone(),
                    "exp_avg_sq": _view_like(bk["v"][off:off + n], p).clone(),
                }
        state = {k: state[k] for k in sorted(state)}
        groups = [{k: v for k, v in self.param_groups[0].items() if k != "params"}]
        groups[0]["no_decay"] = sorted(self._no_decay)
        groups[0]["params"] = list(range(len(self._all_params)))
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """The moments, the step, lr, betas, eps and weight_decay are taken
        from `sd`. The decay MODE (`decoupled`, the `no_decay` set) is this
        optimizer's construction-time choice: a state dict that records
        another one (torch's own records neither) is refused with a
        ValueError before anything is loaded, rather than silently changing
        what weight decay means mid-run."""
        if sd.get("param_groups"):
            src = sd["param_groups"][0]
            if ("decoupled" in src
                    and bool(src["decoupled"]) != self.param_groups[0]["decoupled"]):
                raise ValueError(
                    "FusedAdam: state dict was saved with decoupled=%s, this "
                    "optimizer has decoupled=%s" % (
                        bool(src["decoupled"]),
                        self.param_groups[0]["decoupled"]))
            if ("no_decay" in src
                    and sorted(src["no_decay"]) != sorted(self._no_decay)):
                raise ValueError(
                    "FusedAdam: state dict exempts params %s from weight "
                    "decay, this optimizer %s" % (
                        sorted(src["no_decay"]), sorted(self._no_decay)))
        state = sd.get("state", {})
        steps = []
        for bk in self._materialize():
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                idx = self._index[id(p)]
                ent = state.get(idx, state.get(str(idx)))
                if not ent:
                    continue
                for key, flat in (("exp_avg", bk["m"]), ("exp_avg_sq", bk["v"])):
                    if ent.get(key) is not None:
                        _view_like(flat[off:off + n], p).copy_(
                            ent[key].to(flat.device))
                if ent.get("step") is not None:
                    steps.append(int(float(ent["step"])))
        if steps and self._step_t is not None:
            # one shared counter: every param steps together here
            self._step_t.fill_(max(steps))
        if sd.get("param_groups"):
            src = sd["param_groups"][0]
            g0 = self.param_groups[0]
            for k in ("lr", "eps", "weight_decay"):
                if k in src:
                    g0[k] = float(src[k])
            if "betas" in src:
                g0["betas"] = (float(src["betas"][0]), float(src["betas"][1]))
            if self._lr_dev is not None:
                self._lr_dev.fill_(g0["lr"])
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
