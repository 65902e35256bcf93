"""Child of test_fused_adam_gpu.test_engine_adamw_trains_captured_subprocess
(a fresh process: see test_ops_gpu.test_engine_graph_capture_subprocess).
resnet18_vd, bf16, HIP ops, optimizer="adamw" with no_decay_1d under the
DEFAULT graph-capture policy: 1 eager step, the capture's 3 warm-up steps,
4 replays = 8 optimizer steps on one fixed batch."""
import json
import os
import sys

import torch

sys.path.insert(0, os.environ.get("EDL_REPO") or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))

from edl_amd.train.engine import TrainerEngine  # noqa: E402

eng = TrainerEngine(model="resnet18_vd", per_device_batch=8, num_classes=10,
                    dtype="bf16", base_lr=1e-3, weight_decay=1e-2,
                    use_hip_ops=True, checkpoint_dir=None,
                    optimizer="adamw", no_decay_1d=True).setup()
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
tables = sum(bk["seg_end"] is not None for bk in eng.opt._materialize())
print("RESULT " + json.dumps({
    "captured": captured and eng._graph is not None, "losses": losses,
    "global_step": eng.global_step, "opt_step": eng.opt.step_count,
    "tables": tables, "opt": type(eng.opt).__name__,
}), flush=True)
