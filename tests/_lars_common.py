"""Shared reference, layouts and the tolerance rule of the fused LARS tests
(test_fused_lars_cpu.py, test_fused_lars_gpu.py and their children).

Inputs are _adam_common.make_inputs: params below element 50 are zero (the
pn == 0 branch), every 7th gradient is zero (gn == 0 in a length-1 tensor),
GRAD_SCALE = 0.125 is exact. A LAYOUT is a list of (length, excluded) in
element order; tensor k covers the next `length` elements.

The reference is torch_lars below: Paddle's lars_momentum written out per
tensor in plain torch, run on CPU in fp64 (truth) and in fp32 (yardstick).

The tolerance rule, on the SAME case, over all elements and steps, with
_adam_common.rel_err:
  * p and v:  err(code) <= K * err(torch-fp32), K = 4 (fma contraction and
    another operation order: about one more rounding per operation);
  * trust ratios: relative error against fp64 <= 2^-23. The code sums in
    double (error ~ n * 2^-53) and rounds once to fp32 (2^-24); the factor
    2 of slack is the rule of test_grad_clip_gpu.py.
References are computed once per case (case_reference) and never modified.
At lr=1e-3 the largest parameter move over the six steps is ~0.5 against
|p| >= 0.5 with one sign per element, so nothing cancels to ~0."""
import torch

import _adam_common as A

K = A.K
STEPS = A.STEPS
GRAD_SCALE = A.GRAD_SCALE
TRUST_TOL = 2.0 ** -23
HYPER = dict(lr=1e-3, momentum=0.9, lars_weight_decay=5e-4, lars_coeff=2e-2,
             epsilon=0.0)
# starts at all four offsets mod 4, tensors shorter than a float4, a float4
# over three tensors (elements 1128..1131)
RAGGED = [1, 3, 5, 50, 64, 7, 1000, 1, 2, 4099, 13]


def ragged_layout(excluded=None):
    """RAGGED with every 4th tensor excluded, or the given index set."""
    if excluded is None:
        excluded = {k for k in range(len(RAGGED)) if k % 4 == 3}
    return [(ln, k in excluded) for k, ln in enumerate(RAGGED)]


def spans(layout):
    out, off = [], 0
    for ln, ex in layout:
        out.append((off, off + ln, ex))
        off += ln
    return out


def torch_lars(p0, grads, layout, dtype, lrs=None):
    """-> per step (p, v, trust): p, v flat, trust one entry per tensor.
    Gradients enter pre-scaled by GRAD_SCALE; lrs: per-step LR override."""
    h = HYPER
    p = p0.to(dtype).clone()
    v = torch.zeros_like(p)
    out = []
    for t, g in enumerate(grads):
        g = (g * GRAD_SCALE).to(dtype)
        lr = h["lr"] if lrs is None else lrs[t]
        trust = []
        for s, e, ex in spans(layout):
            wd = 0.0 if ex else h["lars_weight_decay"]
            pn, gn = p[s:e].pow(2).sum().sqrt(), g[s:e].pow(2).sum().sqrt()
            tr = torch.ones((), dtype=dtype)
            if wd > 0 and pn > 0 and gn > 0:
                tr = h["lars_coeff"] * pn / (gn + wd * pn + h["epsilon"])
            v[s:e] = h["momentum"] * v[s:e] + (lr * tr) * (g[s:e] + wd * p[s:e])
            p[s:e] -= v[s:e]
            trust.append(tr)
        out.append((p.clone(), v.clone(), torch.stack(trust)))
    return out


def make_params(layout, p0, device="cpu"):
    """One 1-d fp32 parameter per tensor of the layout, holding its span."""
    return [torch.nn.Parameter(p0[s:e].float().to(device))
            for s, e, _ in spans(layout)]


def make_opt(params, layout, cap_mb=25, **kw):
    """-> (reducer, FusedLARS) over `params` with the layout's exclusions."""
    from edl_amd.ops.lars import FusedLARS
    from edl_amd.train.bucketed_ddp import BucketedAllReducer

    r = BucketedAllReducer(params, bucket_cap_mb=cap_mb)
    kw.setdefault("grad_scale", GRAD_SCALE)
    opt = FusedLARS(params, reducer=r,
                    exclude=[p for p, (_, ex) in zip(params, layout) if ex],
                    **dict(HYPER, **kw))
    return r, opt


def set_grads(params, layout, g):
    for p, (s, e, _) in zip(params, spans(layout)):
        p.grad.copy_(g[s:e].to(p.dtype))


def opt_state(params, opt):
    """(p, v, trust) of a FusedLARS in the layout's element order, on CPU."""
    sd = opt.state_dict()["state"]
    return (torch.cat([p.detach().reshape(-1) for p in params]).cpu(),
            torch.cat([sd[i]["velocity"].reshape(-1)
                       for i in range(len(params))]).cpu(),
            opt.trust_ratios().clone().cpu())


def run_opt(params, layout, opt, grads, clip_state=None):
    out = []
    for g in grads:
        set_grads(params, layout, g)
        opt.step(clip_state=clip_state)
        out.append(opt_state(params, opt))
    return out


def run_errors(run, truth_run):
    """-> {"p", "v", "trust"}: largest rel_err over the steps."""
    out = {"p": 0.0, "v": 0.0, "trust": 0.0}
    for got, truth in zip(run, truth_run):
        for k, x, t in zip(("p", "v", "trust"), got, truth):
            out[k] = max(out[k], A.rel_err(x, t))
    return out


_REFS = {}


def case_reference(layout, offset=0, steps=STEPS, lrs=None):
    """-> (p0, grads, truth_run, torch-fp32's {"p","v","trust"} errors) of
    the case, computed once."""
    key = (tuple(layout), offset, steps, None if lrs is None else tuple(lrs))
    if key not in _REFS:
        n = sum(ln for ln, _ in layout)
        p0, grads = A.make_inputs(n, offset)
        grads = grads[:steps]
        truth = torch_lars(p0, grads, layout, torch.float64, lrs)
        f32 = torch_lars(p0, grads, layout, torch.float32, lrs)
        _REFS[key] = (p0, grads, truth, run_errors(f32, truth))
    return _REFS[key]


def check(errs, ref_errs, what):
    """The tolerance rule; prints every figure before asserting."""
    for k in "pv":
        ratio = (errs[k] / ref_errs[k]) if ref_errs[k] > 0 else (
            0.0 if errs[k] == 0 else float("inf"))
        print("LARS_TOL %s %s: err %.3e torch-fp32 %.3e ratio %.2f"
              % (what, k, errs[k], ref_errs[k], ratio))
    print("LARS_TOL %s trust: err %.3e bound %.3e (torch-fp32 %.3e)"
          % (what, errs["trust"], TRUST_TOL, ref_errs["trust"]))
    for k in "pv":
        assert errs[k] <= K * ref_errs[k], (what, k, errs[k], ref_errs[k])
    assert errs["trust"] <= TRUST_TOL, (what, errs["trust"])
