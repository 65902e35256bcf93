"""Shared inputs, references and the tolerance rule of the fused Adam tests
(test_fused_adam_cpu.py, test_fused_adam_gpu.py).

Inputs are a function of the ELEMENT INDEX, not of n, so a smaller case is
a prefix of a larger one:
  * gradients span 1e-6 .. 1e2 in magnitude, cycling through the decades
    every PERIOD elements; element i keeps one sign over all steps and its
    magnitude changes smoothly per step; every 7th gradient is zero;
  * the first 50 params are zero, the rest have 0.5 <= |p| < 2;
  * grad_scale = 0.125 (exact in binary: the references take pre-scaled
    gradients), steps t = 1..6.
One sign per element and |p| >= 0.5 keep p away from cancelling to ~0
(six steps at lr 1e-3 move it by at most ~6e-3): a relative error measured
at a cancelled element is a lottery between two roundings, not a property
of the code.

The tolerance rule. torch.optim.Adam / AdamW (foreach=False) run on CPU in
fp64 (truth) and in fp32. With
    err(x) = max(|x - truth| / max(|truth|, 1e-30))
over the elements and the six steps, for each of p, m, v the code under
test must satisfy err(code) <= K * err(torch-fp32), K = 4: the headroom
covers fma contraction and another sqrt/div order, about one more rounding
per operation. Both errors are taken on the SAME case: a case of n elements
is held to K times torch-fp32's error over those n elements, however few.
The references of a case are computed once (case_reference caches them)
and never modified."""
import math

import torch

K = 4.0
STEPS = 6
GRAD_SCALE = 0.125
PERIOD = 1021  # prime: decades do not line up with float4 lanes or blocks
N_REF = (1 << 20) + 3
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
WD = {"l2": 1e-2, "decoupled": 1e-2}


def make_inputs(n, offset=0):
    """-> p0 [n] fp64, grads: STEPS tensors [n] fp64 (UNSCALED: the code
    under test multiplies by GRAD_SCALE). All values are fp32-exact."""
    i = torch.arange(offset, offset + n, dtype=torch.float64)
    frac = (i % PERIOD) / (PERIOD - 1)
    mag = 10.0 ** (-6.0 + 8.0 * frac)
    sign = 1.0 - 2.0 * ((i * 7919) % 2)
    mant = 1.0 + ((i * 2654435761) % 1000) / 1000.0
    base = sign * mag * mant
    base[(i % 7) == 6] = 0.0
    grads = [(base * (1.0 + 0.25 * math.sin(1.0 + t))).float().double()
             for t in range(STEPS)]
    psign = 1.0 - 2.0 * ((i * 104729) % 2)
    p0 = psign * (0.5 + 1.5 * ((i * 40503) % 4096) / 4096.0)
    p0[i < 50] = 0.0
    return p0.float().double(), grads


def torch_run(p0, grads, mode, dtype, groups=None, weight_decay=None):
    """torch.optim.Adam (mode "l2") / AdamW ("decoupled") on CPU over one
    flat param — or over `groups`, a list of (start, end, wd) slices, as
    separate params in per-decay param groups. Gradients enter pre-scaled
    by GRAD_SCALE. -> per step (p, m, v), each flat, in `dtype`."""
    wd = WD[mode] if weight_decay is None else weight_decay
    if groups is None:
        groups = [(0, p0.numel(), wd)]
    params = [torch.nn.Parameter(p0[s:e].to(dtype).clone())
              for s, e, _ in groups]
    cls = torch.optim.Adam if mode == "l2" else torch.optim.AdamW
    opt = cls([{"params": [p], "weight_decay": g[2]}
               for p, g in zip(params, groups)], foreach=False, **HYPER)
    out = []
    for g in grads:
        for p, (s, e, _) in zip(params, groups):
            p.grad = (g[s:e] * GRAD_SCALE).to(dtype)
        opt.step()
        out.append(tuple(
            torch.cat([pick(p) for p in params]).clone()
            for pick in (lambda p: p.detach(),
                         lambda p: opt.state[p]["exp_avg"],
                         lambda p: opt.state[p]["exp_avg_sq"])))
    return out


def rel_err(x, truth):
    x = x.detach().double().cpu()
    if x.numel() == 0:
        return 0.0
    return float(((x - truth).abs() / truth.abs().clamp_min(1e-30)).max())


def run_errors(run, truth_run, n=None):
    """-> {"p", "m", "v"}: err over the first n elements and all steps."""
    out = {"p": 0.0, "m": 0.0, "v": 0.0}
    for got, truth in zip(run, truth_run):
        for k, x, t in zip("pmv", got, truth):
            if n is not None:
                x, t = x[:n], t[:n]
            out[k] = max(out[k], rel_err(x, t))
    return out


_REFS = {}


def case_reference(n, mode):
    """Truth (fp64) run and torch-fp32's errors of the n-element uniform
    case itself, computed once. -> (truth_run, {"p","m","v"})."""
    if (n, mode) not in _REFS:
        p0, grads = make_inputs(n)
        truth = torch_run(p0, grads, mode, torch.float64)
        f32 = torch_run(p0, grads, mode, torch.float32)
        _REFS[(n, mode)] = (truth, run_errors(f32, truth))
    return _REFS[(n, mode)]


def check(errs, ref_errs, what):
    """The tolerance rule; prints every figure before asserting."""
    ratios = {}
    for k in "pmv":
        ratios[k] = (errs[k] / ref_errs[k]) if ref_errs[k] > 0 else (
            0.0 if errs[k] == 0 else float("inf"))
        print("ADAM_TOL %s %s: err %.3e torch-fp32 %.3e ratio %.2f"
              % (what, k, errs[k], ref_errs[k], ratios[k]))
    for k in "pmv":
        assert errs[k] <= K * ref_errs[k], (what, k, errs[k], ref_errs[k])
    return ratios
