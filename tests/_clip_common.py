"""Shared pieces of the gradient-clipping tests (test_grad_clip_cpu.py,
test_grad_clip_gpu.py, their workers and children).

The model and the inputs are those of the fused Adam tests (_adam_common:
index-defined gradients spanning 1e-6..1e2, every 7th zero, grad_scale =
0.125), each step's gradient additionally multiplied by FACTORS[t] so the
global norm straddles max_norm: MAX_NORM_REL times the fp64 norm of the
first step's averaged gradient is the bound, so steps with a factor above
it are clipped and the others are not. The numeric rule is _adam_common's
(K times torch-fp32's own error against the fp64 truth of the same case);
the truth and the yardstick are torch.nn.utils.clip_grad_norm_ followed by
torch.optim on CPU."""
import torch

import _adam_common as C

# per-step multipliers (powers of two: exact) around MAX_NORM_REL
FACTORS = [0.5, 2.0, 0.25, 4.0, 1.0, 8.0]
MAX_NORM_REL = 1.5  # relative to step 0's norm BEFORE its factor
SGD = dict(lr=1e-3, momentum=0.9, weight_decay=1e-2)


def model(dtype=torch.float32, device="cpu"):
    """The two-layer model of test_fused_adam_cpu with _adam_common's
    index-defined params. -> (model, the six factor-scaled gradients)."""
    m = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(),
                            torch.nn.Linear(64, 4)).to(dtype)
    n = sum(p.numel() for p in m.parameters())
    p0, grads = C.make_inputs(n)
    off = 0
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p0[off:off + p.numel()].view_as(p))
            off += p.numel()
    return m.to(device), [g * f for g, f in zip(grads, FACTORS)]


def max_norm_for(grads):
    """The bound of a run, from the inputs alone (fp64)."""
    base = float((grads[0] / FACTORS[0] * C.GRAD_SCALE).norm())
    return MAX_NORM_REL * base


def clipped_steps(grads, max_norm):
    return [float((g * C.GRAD_SCALE).norm()) > max_norm for g in grads]


def set_grads(m, flat, scale=1.0):
    off = 0
    for p in m.parameters():
        g = (flat[off:off + p.numel()] * scale).view_as(p).to(
            device=p.device, dtype=p.dtype)
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)
        off += p.numel()


def make_torch_opt(m, kind):
    if kind == "sgd":
        return torch.optim.SGD(m.parameters(), foreach=False, **SGD)
    cls = torch.optim.Adam if kind == "adam" else torch.optim.AdamW
    mode = "l2" if kind == "adam" else "decoupled"
    return cls(m.parameters(), foreach=False, weight_decay=C.WD[mode],
               **C.HYPER)


def torch_state(m, opt, kind):
    """(p, m, v) flat in parameters() order; SGD has no v: its momentum
    buffer stands in twice so _adam_common's three-way rule applies."""
    ps = list(m.parameters())
    flat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs]).clone()
    if kind == "sgd":
        mom = flat([opt.state[p]["momentum_buffer"] for p in ps])
        return flat(ps), mom, mom
    return (flat(ps), flat([opt.state[p]["exp_avg"] for p in ps]),
            flat([opt.state[p]["exp_avg_sq"] for p in ps]))


def torch_run(kind, dtype, grads, max_norm, skip_steps=()):
    """clip_grad_norm_ + torch.optim on CPU; gradients enter pre-scaled by
    GRAD_SCALE (exact). Steps listed in skip_steps are never seen.
    -> per applied step (p, m, v)."""
    m, _ = model(dtype)
    opt = make_torch_opt(m, kind)
    out = []
    for t, g in enumerate(grads):
        if t in skip_steps:
            continue
        set_grads(m, g, C.GRAD_SCALE)
        torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm,
                                       foreach=False)
        opt.step()
        out.append(torch_state(m, opt, kind))
    return out


def make_fused(m, kind, max_norm, skip_nonfinite=False, grad_scale=None):
    """-> (reducer, optimizer, clipper) over m's params."""
    from edl_amd.ops.adam import FusedAdam, FusedAdamW
    from edl_amd.ops.clip import GradClipper
    from edl_amd.ops.sgd import FusedSGD
    from edl_amd.train.bucketed_ddp import BucketedAllReducer

    r = BucketedAllReducer(m.parameters(), bucket_cap_mb=25)
    gs = C.GRAD_SCALE if grad_scale is None else grad_scale
    if kind == "sgd":
        opt = FusedSGD(m.parameters(), grad_scale=gs, reducer=r, **SGD)
    elif kind == "adam":
        opt = FusedAdam(m.parameters(), weight_decay=C.WD["l2"],
                        grad_scale=gs, reducer=r, **C.HYPER)
    else:
        opt = FusedAdamW(m.parameters(), weight_decay=C.WD["decoupled"],
                         grad_scale=gs, reducer=r, **C.HYPER)
    return r, opt, GradClipper(r, max_norm, skip_nonfinite)


def fused_state(m, opt, kind):
    ps = list(m.parameters())
    flat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs]).cpu()
    if kind == "sgd":
        # FusedSGD's state dict counts in bucket order: read the momentum
        # slices by param instead
        by_param = {}
        for bk in opt._materialize():
            for (off, n), p in zip(bk["offsets"], bk["params"]):
                by_param[id(p)] = bk["m"][off:off + n].clone()
        mom = flat([by_param[id(p)] for p in ps])
        return flat(ps), mom, mom
    sd = opt.state_dict()["state"]
    return (flat(ps), flat([sd[i]["exp_avg"] for i in range(len(ps))]),
            flat([sd[i]["exp_avg_sq"] for i in range(len(ps))]))


def fused_step(m, opt, clipper, g):
    """One clipped step on unscaled gradients -> the clip state."""
    set_grads(m, g)
    st = clipper.run(opt.grad_scale)
    opt.step(clip_state=st)
    return st
