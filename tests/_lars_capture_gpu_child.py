"""Child of test_fused_lars_gpu.test_graph_capture_subprocess (a fresh
process: see test_ops_gpu.test_engine_graph_capture_subprocess). ONE
FusedLARS step over the ragged layout (several buckets, a GradClipper in
norm-only mode in front) is captured and replayed 3 times with new
gradients each time and a new LR before the third; the references are 3
eager steps of _lars_common.torch_lars on CPU (fp64 truth, fp32
yardstick)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.environ.get("EDL_REPO") or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))

import _adam_common as A  # noqa: E402
import _lars_common as L  # noqa: E402
from edl_amd import ops  # noqa: E402
from edl_amd.ops.clip import GradClipper  # noqa: E402

assert ops.available(), "edl_amd._C missing on a GPU box"
LR3 = 4e-3  # the LR of the third step


def main():
    layout = L.ragged_layout()
    lrs = [L.HYPER["lr"], L.HYPER["lr"], LR3]
    p0, grads, truth, ref = L.case_reference(layout, steps=3, lrs=lrs)

    # load the kernels outside the capture, on tensors the captured
    # optimizer does not own
    warm = L.make_params([(5, False), (3, True)], p0, "cuda")
    wr, wopt = L.make_opt(warm, [(5, False), (3, True)])
    wclip = GradClipper(wr, None, True)
    wopt.step(clip_state=wclip.run(wopt.grad_scale))
    torch.cuda.synchronize()

    params = L.make_params(layout, p0, "cuda")
    r, opt = L.make_opt(params, layout, cap_mb=0.004)
    clipper = GradClipper(r, None, True)  # norm only: coef stays 1
    opt._materialize()  # tables are built (H2D copies) before the capture
    clipper._materialize()
    L.set_grads(params, layout, grads[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(clip_state=clipper.run(opt.grad_scale))
    torch.cuda.synchronize()
    v_after_capture = max(float(v.abs().max()) for v in opt.state_buffers())
    got = []
    for t, g in enumerate(grads):
        if t == 2:
            opt.set_lr(LR3)
        L.set_grads(params, layout, g)
        graph.replay()
        torch.cuda.synchronize()
        got.append(L.opt_state(params, opt))

    # what the third step would have been at the OLD lr: must be far off
    h = L.HYPER
    v_old = h["momentum"] * truth[1][1] + (
        truth[2][1] - h["momentum"] * truth[1][1]) * (h["lr"] / LR3)
    print("RESULT " + json.dumps({
        "buckets": len(r._buckets), "v_after_capture": v_after_capture,
        "errs": L.run_errors(got, truth), "ref": ref,
        "trust_changed": [not torch.equal(got[i][2], got[i + 1][2])
                          for i in range(2)],
        "lr_gap": A.rel_err(got[2][0], truth[1][0] - v_old),
        "skipped": float(clipper.skipped.item()),
    }), flush=True)


main()
