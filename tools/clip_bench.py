#!/usr/bin/env python3
"""Time the global gradient norm + clip state (csrc/grad_norm.hip) on flat
fp32 buffers:

    python tools/clip_bench.py

  sumsq       grad_sumsq alone: one read stream of 4 B per element
  clip        grad_sumsq + grad_clip_finalize, what GradClipper.run launches
  fused_sgd   the momentum kernel on the same n: the streaming yardstick
              (5 streams of 4 B per element against the reduction's 1)
  torch_clip  torch.nn.utils.clip_grad_norm_(foreach=True) over 160 views
              of the same storage (what one would run without the flat
              buckets; it also rescales the gradients in place, which the
              fused path folds into the update kernel)

The variants alternate within each repeat. A figure is the median over
repeats of (event time of ITERS back-to-back launches) / ITERS, with
min..max, in microseconds; *_gbs is the byte model over the median.

--segments S splits the n elements into S buffers reduced in one call
(ceil(S/16) launches): S buffers get S times the row cap, which is how the
cap (GRAD_NORM_ROW_CAP rows of 256 threads per buffer) is sized.

--rotate R gives the HIP variants R independent buffer sets and launch i
works on set i % R, so with R x (bytes per set) far above the 256 MB L3
every launch starts cache-cold, as the clip of a training step does after
a forward and a backward pass. torch_clip is left out of a rotated run.

    python tools/clip_bench.py --sizes 25557032 --rotate 6
    python tools/clip_bench.py --sizes 102228128     # far beyond the L3

Prints one JSON line per n."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from edl_amd.ops import ext  # noqa: E402

NVIEWS = 160


def time_us(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def split(flat, parts):
    """`parts` contiguous 16-byte aligned slices covering flat."""
    n = flat.numel()
    step = max(4, (n // parts) // 4 * 4)
    cuts = [min(n, k * step) for k in range(parts)] + [n]
    return [flat[a:b] for a, b in zip(cuts, cuts[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--sizes", default="6553600,25557032,65536")
    ap.add_argument("--rotate", type=int, default=1,
                    help="independent buffer sets cycled per launch")
    ap.add_argument("--segments", type=int, default=1,
                    help="buffers the n elements are split into")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    e = ext()
    lr, wd, mu = 1e-3, 1e-2, 0.9

    for n in (int(x) for x in args.sizes.split(",")):
        gen = torch.Generator(device="cuda").manual_seed(0)
        p, g = (torch.randn(n, device="cuda", generator=gen) for _ in range(2))
        m = torch.zeros_like(p)
        lr_dev = torch.full((1,), lr, device="cuda")
        state = torch.zeros(4, device="cuda")
        sets = [(p, g, m)] + [(p.clone(), g.clone(), m.clone())
                              for _ in range(args.rotate - 1)]
        segs = [split(s[1], args.segments) for s in sets]
        rows = sum(e.grad_norm_rows(b.numel()) for b in segs[0])
        partial = torch.empty(rows, dtype=torch.float64, device="cuda")
        # torch's clip over views of its own copy (it rescales in place)
        views = []
        for t in split(g.clone(), NVIEWS):
            w = torch.empty_like(t).requires_grad_(True)
            w.grad = t
            views.append(w)
        turn = [0]

        def nxt():
            turn[0] += 1
            return turn[0] % len(sets)

        def sumsq():
            e.grad_sumsq(segs[nxt()], partial)

        def clip():
            r = e.grad_sumsq(segs[nxt()], partial)
            e.grad_clip_finalize(partial, r, state, 1.0, 1.0, True)

        def fused_sgd():
            sp, sg, sm = sets[nxt()]
            e.fused_sgd(sp, sg, sm, lr, mu, wd, 1.0, lr_dev)

        def torch_clip():
            torch.nn.utils.clip_grad_norm_(views, 1.0, foreach=True)

        variants = {"sumsq": sumsq, "clip": clip, "fused_sgd": fused_sgd}
        if args.rotate == 1:
            variants["torch_clip"] = torch_clip
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                samples[name].append(time_us(fn, args.iters))
        out = {"n": n, "segments": args.segments, "rows": rows,
               "iters": args.iters, "repeats": args.repeats,
               "rotate": args.rotate}
        # torch_clip: norm pass (read) + rescale pass (read + write)
        streams = {"sumsq": 1, "clip": 1, "fused_sgd": 5, "torch_clip": 3}
        for name, s in samples.items():
            med = statistics.median(s)
            out[name + "_us"] = [round(med, 1), round(min(s), 1),
                                 round(max(s), 1)]
            out[name + "_gbs"] = round(streams[name] * 4 * n / med / 1e3, 1)
        out["clip_over_fused_sgd"] = round(
            out["clip_us"][0] / out["fused_sgd_us"][0], 3)
        out["model_clip_over_fused_sgd"] = round(1 / 5, 2)
        if "torch_clip_us" in out:
            out["torch_over_clip"] = round(
                out["torch_clip_us"][0] / out["clip_us"][0], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
