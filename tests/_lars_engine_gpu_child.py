"""Child of test_fused_lars_gpu.test_engine_lars_trains_captured_subprocess
(a fresh process: see test_ops_gpu.test_engine_graph_capture_subprocess).
resnet18_vd, bf16, HIP ops, optimizer="lars" with no_decay_1d and
clip_grad_norm under the DEFAULT graph-capture policy: 1 eager step, the
capture's 3 warm-up steps, 4 replays = 8 optimizer steps on one fixed
batch."""
import json
import os
import sys

import torch

sys.path.insert(0, os.environ.get("EDL_REPO") or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))

from edl_amd.train.engine import TrainerEngine  # noqa: E402

eng = TrainerEngine(model="resnet18_vd", per_device_batch=8, num_classes=10,
                    dtype="bf16", base_lr=0.05, weight_decay=5e-4,
                    use_hip_ops=True, checkpoint_dir=None,
                    optimizer="lars", lars_coeff=0.02, no_decay_1d=True,
                    clip_grad_norm=10.0, skip_nonfinite=True).setup()
g = torch.Generator().manual_seed(0)
x = torch.randn(8, 3, 64, 64, generator=g).cuda().contiguous(
    memory_format=torch.channels_last)
y = torch.randint(0, 10, (8,), generator=g).cuda()
eng.model.train()
losses = [float(eng.train_step(x, y).item())]
captured = bool(eng.maybe_capture(x, y))
for _ in range(4):
    loss = eng.replay_step(x, y)
    torch.cuda.synchronize()
    losses.append(float(loss.item()))
tr = eng.last_trust_ratios.cpu()
ex = [i for i, p in enumerate(eng.model.parameters()) if p.ndim <= 1]
print("RESULT " + json.dumps({
    "captured": captured and eng._graph is not None, "losses": losses,
    "global_step": eng.global_step, "opt": type(eng.opt).__name__,
    "trust_excluded_all_one": bool((tr[ex] == 1).all()),
    "trust_moved": bool((tr != 1).any()),
    "trust_min_max": [float(tr.min()), float(tr.max())],
    "grad_norm": float(eng.last_grad_norm.item()),
    "skipped": float(eng.skipped_steps.item()),
}), flush=True)
