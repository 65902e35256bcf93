"""Child of test_grad_clip_gpu.test_graph_capture_subprocess (a fresh
process, one stream). GradClipper.run (reduce + finalize) and ONE
FusedAdamW step are captured together and replayed 4 times, the gradient
buffers rewritten between replays: below max_norm, above it, holding one
inf (skip_nonfinite on), below again. The references are the three APPLIED
steps as eager torch on CPU: clip_grad_norm_ + AdamW (fp64 truth, fp32
yardstick)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.environ.get("EDL_REPO") or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _adam_common as C  # noqa: E402
import _clip_common as CC  # noqa: E402
from edl_amd import ops  # noqa: E402

assert ops.available(), "edl_amd._C missing on a GPU box"


def main():
    dev = torch.device("cuda")
    ext = ops.ext()
    # load the kernels and the counter's ops outside the capture, on
    # tensors the optimizer and the clipper do not own
    w = [torch.zeros(8, device=dev) for _ in range(4)]
    wt = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(4, device=dev)
    wp = torch.empty(1, dtype=torch.float64, device=dev)
    ext.grad_clip_finalize(wp, ext.grad_sumsq([w[1]], wp), ws, 1.0, 1.0, True)
    wt.add_((1.0 - ws[2:3]).to(torch.int32))
    ext.fused_adam(*w, wt, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, False, None,
                   None, None, ws)
    torch.cuda.synchronize()

    m, grads = CC.model(torch.float32, dev)
    max_norm = CC.max_norm_for(grads)
    bad = grads[2].clone()
    bad[77] = float("inf")
    seq = [grads[0], grads[1], bad, grads[4]]
    applied = [grads[0], grads[1], grads[4]]
    assert CC.clipped_steps(applied, max_norm) == [False, True, False]
    _, opt, clipper = CC.make_fused(m, "adamw", max_norm,
                                    skip_nonfinite=True)
    opt._materialize()
    clipper._materialize()
    CC.set_grads(m, seq[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(clip_state=clipper.run(opt.grad_scale))
    torch.cuda.synchronize()
    step_after_capture = opt.step_count  # a capture runs nothing
    got, coef_lt_1, skip = [], [], []
    unchanged = None
    for t, g in enumerate(seq):
        before = CC.fused_state(m, opt, "adamw")
        CC.set_grads(m, g)
        graph.replay()
        torch.cuda.synchronize()
        st = clipper.state.cpu()
        coef_lt_1.append(bool(st[0] < 1.0) and t != 2)
        skip.append(float(st[2]))
        after = CC.fused_state(m, opt, "adamw")
        if t == 2:
            unchanged = all(torch.equal(a, b) for a, b in zip(before, after))
        else:
            got.append(after)

    truth = CC.torch_run("adamw", torch.float64, applied, max_norm)
    ref = C.run_errors(CC.torch_run("adamw", torch.float32, applied,
                                    max_norm), truth)
    print("RESULT " + json.dumps({
        "step_after_capture": step_after_capture, "step": opt.step_count,
        "nskipped": float(clipper.skipped), "coef_lt_1": coef_lt_1,
        "skip": skip, "skipped_step_unchanged": unchanged,
        "errs": C.run_errors(got, truth), "ref": ref,
    }), flush=True)


main()
