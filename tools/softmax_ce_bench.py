#!/usr/bin/env python3
"""Time the fused softmax-CE (forward + backward) against the path it
replaces in the engine, F.cross_entropy(logits.float(), y,
label_smoothing=0.1) forward + backward, on bf16 logits.

    python tools/softmax_ce_bench.py --mode eager
    python tools/softmax_ce_bench.py --mode graph   # one process per mode

eager: host-launched, so it includes the launch cost of every kernel in
the chain. graph: the same work captured as one hipGraph and replayed,
which is how the benchmark's train step runs it. The two variants
alternate within each repeat; the figure is the median over repeats of
(event time of ITERS back-to-back iterations) / ITERS. Prints one JSON
line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from edl_amd.ops.functional import softmax_cross_entropy  # noqa: E402


def make_step(kind, logits, labels):
    if kind == "fused":
        def step():
            logits.grad = None
            softmax_cross_entropy(logits, labels, label_smoothing=0.1).backward()
    else:
        def step():
            logits.grad = None
            F.cross_entropy(logits.float(), labels,
                            label_smoothing=0.1).backward()
    return step


def time_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=["eager", "graph"], default="eager")
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--repeats", type=int, default=21)
    p.add_argument("--warmup", type=int, default=50)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"

    for B, C in ((32, 1000), (256, 1000)):
        torch.manual_seed(0)
        runs = {}
        for kind in ("fused", "torch"):
            logits = (torch.randn(B, C, device="cuda") * 4).to(
                torch.bfloat16).requires_grad_(True)
            labels = torch.randint(0, C, (B,), device="cuda")
            step = make_step(kind, logits, labels)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(args.warmup):
                    step()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            if args.mode == "graph":
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    step()
                runs[kind] = (g.replay, logits)
            else:
                runs[kind] = (step, logits)
        for fn, _ in runs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in runs}
        for _ in range(args.repeats):
            for kind, (fn, _) in runs.items():
                samples[kind].append(time_ms(fn, args.iters))
        out = {"mode": args.mode, "shape": [B, C], "dtype": "bf16",
               "iters": args.iters, "repeats": args.repeats}
        for kind, v in samples.items():
            out[kind + "_us_median"] = round(statistics.median(v) * 1e3, 2)
            out[kind + "_us_min"] = round(min(v) * 1e3, 2)
            out[kind + "_us_max"] = round(max(v) * 1e3, 2)
        out["torch_over_fused"] = round(
            out["torch_us_median"] / out["fused_us_median"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
