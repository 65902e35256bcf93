"""Child of test_fused_adam_gpu.test_graph_capture_subprocess (a fresh
process: see test_ops_gpu.test_engine_graph_capture_subprocess). ONE
FusedAdamW step with a decay table is captured and replayed 3 times with
new gradients each time and a new LR before the third; the references are
3 eager torch AdamW steps on CPU (fp64 truth, fp32 yardstick)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.environ.get("EDL_REPO") or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))

import _adam_common as C  # noqa: E402
from edl_amd import ops  # noqa: E402
from edl_amd.ops.adam import FusedAdamW  # noqa: E402
from edl_amd.train.bucketed_ddp import BucketedAllReducer  # noqa: E402

assert ops.available(), "edl_amd._C missing on a GPU box"
LR3 = 4e-3  # the LR of the third step


def model(dtype, device):
    m = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(),
                            torch.nn.Linear(64, 4)).to(dtype)
    n = sum(p.numel() for p in m.parameters())
    p0, grads = C.make_inputs(n)
    off = 0
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p0[off:off + p.numel()].view_as(p))
            off += p.numel()
    return m.to(device), grads


def set_grads(m, flat, scale):
    off = 0
    for p in m.parameters():
        g = (flat[off:off + p.numel()] * scale).view_as(p)
        if p.grad is None:
            p.grad = torch.empty_like(p)
        p.grad.copy_(g.to(p.dtype))
        off += p.numel()


def flat_state(m, state):
    ps = list(m.parameters())
    return tuple(torch.cat([f(i, p).reshape(-1) for i, p in enumerate(ps)])
                 for f in (lambda i, p: p.detach(),
                           lambda i, p: state(i, p)["exp_avg"],
                           lambda i, p: state(i, p)["exp_avg_sq"]))


def torch_run(dtype, grads):
    m, _ = model(dtype, "cpu")
    ps = list(m.parameters())
    opt = torch.optim.AdamW(
        [{"params": [p for p in ps if p.ndim > 1]},
         {"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0.0}],
        foreach=False, weight_decay=C.WD["decoupled"], **C.HYPER)
    out = []
    for t, g in enumerate(grads):
        if t == 2:
            for grp in opt.param_groups:
                grp["lr"] = LR3
        set_grads(m, g, C.GRAD_SCALE)
        opt.step()
        out.append(flat_state(m, lambda i, p: opt.state[p]))
    return out


def main():
    dev = torch.device("cuda")
    # load the kernel and the counter's add_ outside the capture, on
    # tensors the optimizer does not own
    w = [torch.zeros(8, device=dev) for _ in range(4)]
    wt = torch.zeros(1, dtype=torch.int32, device=dev)
    wt.add_(1)
    ops.ext().fused_adam(*w, wt, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, False)
    torch.cuda.synchronize()

    mf, grads = model(torch.float32, dev)
    grads = grads[:3]
    r = BucketedAllReducer(mf.parameters(), bucket_cap_mb=25)
    opt = FusedAdamW(mf.parameters(), weight_decay=C.WD["decoupled"],
                     no_decay=lambda p: p.ndim <= 1,
                     grad_scale=C.GRAD_SCALE, reducer=r, **C.HYPER)
    bk = opt._materialize()[0]
    has_table = bk["seg_end"] is not None
    set_grads(mf, grads[0], 1.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    step_after_capture = opt.step_count  # a capture runs nothing
    got = []
    for t, g in enumerate(grads):
        if t == 2:
            opt.set_lr(LR3)
        set_grads(mf, g, 1.0)
        graph.replay()
        torch.cuda.synchronize()
        sd = opt.state_dict()["state"]
        got.append(tuple(x.cpu() for x in flat_state(mf, lambda i, p: sd[i])))

    truth = torch_run(torch.float64, grads)
    ref = C.run_errors(torch_run(torch.float32, grads), truth)
    errs = C.run_errors(got, truth)
    # what the third step would have been at the OLD lr: must be far off
    p_old_lr = truth[1][0] + (truth[2][0] - truth[1][0]) * (C.HYPER["lr"] / LR3)
    print("RESULT " + json.dumps({
        "has_table": has_table, "step_after_capture": step_after_capture,
        "step": opt.step_count,
        "sd_step": float(opt.state_dict()["state"][0]["step"]),
        "errs": errs, "ref": ref,
        "lr_gap": C.rel_err(got[2][0], p_old_lr),
    }), flush=True)


main()
