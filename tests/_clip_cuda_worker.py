"""Worker for test_grad_clip_gpu.test_two_ranks_one_gpu: 2 ranks sharing
cuda:0 (gloo collectives, EDL_FORCE_BACKEND=gloo) train
TrainerEngine(optimizer="adamw", clip_grad_norm=...) for 4 steps on
per-rank data. Every rank reduces the same all-reduced buckets with the
same deterministic kernels, so with no collective of its own the clip
state must agree bit for bit: last_grad_norm after every step and the
params at the end are compared across the ranks."""
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from edl_amd.train.engine import TrainerEngine  # noqa: E402

MAX_NORM = 0.25


def same_on_all_ranks(t, world):
    t = t.detach().cpu().contiguous()
    got = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(got, t)
    return all(torch.equal(got[0], x) for x in got[1:])


def main():
    rank = int(os.environ["RANK"])
    eng = TrainerEngine(
        model="mnist_mlp", per_device_batch=8, num_classes=10, base_lr=1e-3,
        weight_decay=1e-2, label_smoothing=0.0, dtype="fp32",
        channels_last=False, checkpoint_dir=None, optimizer="adamw",
        clip_grad_norm=MAX_NORM, skip_nonfinite=True).setup()
    world = dist.get_world_size()
    ok, detail, clipped = world == 2, "", 0
    gen = torch.Generator().manual_seed(100 + rank)  # per-rank data
    for s in range(4):
        x = torch.randn(8, 1, 28, 28, generator=gen).to(eng.device)
        y = torch.randint(0, 10, (8,), generator=gen).to(eng.device)
        eng.train_step(x, y)
        st = eng.clipper.state.clone()
        if not same_on_all_ranks(st, world):
            ok, detail = False, "clip state differs at step %d" % s
        if not same_on_all_ranks(eng.last_grad_norm, world):
            ok, detail = False, "last_grad_norm differs at step %d" % s
        if not float(st[1]) > 0:
            ok, detail = False, "norm %r at step %d" % (float(st[1]), s)
        clipped += int(float(st[0]) < 1.0)
    if not (eng.clipper.state.is_cuda and eng.last_grad_norm.is_cuda):
        ok, detail = False, "clip state is not on the GPU"
    for b in eng.reducer._buckets:
        if not same_on_all_ranks(b.param_flat, world):
            ok, detail = False, "params differ across ranks"
    if eng.opt.step_count != 4 or float(eng.skipped_steps) != 0.0:
        ok, detail = False, "step count / skipped"
    dist.barrier()
    dist.destroy_process_group()
    print(json.dumps({"clip_cuda": True, "rank": rank, "ok": ok,
                      "clipped": clipped, "detail": detail}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
