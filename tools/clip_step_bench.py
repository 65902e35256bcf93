#!/usr/bin/env python3
"""bench.py's single-GPU workload with gradient clipping switched on:

    python tools/clip_step_bench.py --steps 60 --warmup 15
    python tools/clip_step_bench.py --clip_grad_norm none    # the plain step

ResNet50_vd, 32 per GPU, bf16, the default capture policy, W untimed steps
then K timed ones, exactly as bench.py times them, but with
TrainerEngine(clip_grad_norm=..., skip_nonfinite=True). bench.py itself
never clips; the cost of the feature per step is this tool's ms_per_step
with a bound minus its ms_per_step with `none`, runs of the two
alternating (one process each: one graph capture per process).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from edl_amd.data.synthetic import SyntheticImageNet  # noqa: E402
from edl_amd.train.engine import TrainerEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--model", default="resnet50_vd")
    ap.add_argument("--clip_grad_norm", default="1.0",
                    help="the bound, or `none` for the plain step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    clip = args.clip_grad_norm.lower() != "none"
    kw = {}
    if clip:
        kw = dict(clip_grad_norm=float(args.clip_grad_norm),
                  skip_nonfinite=True)
    engine = TrainerEngine(
        model=args.model, per_device_batch=args.batch_size, base_lr=0.1,
        dtype="bf16", channels_last=True, checkpoint_dir=None,
        use_hip_ops=True, **kw).setup()
    engine.model.train()
    engine.set_lr(engine.scaled_lr(0))
    loader = SyntheticImageNet(args.batch_size, engine.device,
                               channels_last=True, seed=1234)
    x, y = loader.next()
    captured = engine.maybe_capture(x, y)
    for _ in range(max(1, args.warmup)):
        engine.replay_step(*loader.next())
    torch.cuda.synchronize()
    t0 = time.monotonic()
    for _ in range(args.steps):
        engine.replay_step(*loader.next())
    torch.cuda.synchronize()
    ms = (time.monotonic() - t0) / args.steps * 1e3
    out = {"clip_grad_norm": args.clip_grad_norm, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(ms, 3),
           "img_per_s": round(args.batch_size / ms * 1e3, 1),
           "graph_capture": bool(captured)}
    if clip:
        out["last_grad_norm"] = float(engine.last_grad_norm)
        out["skipped_steps"] = float(engine.skipped_steps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
