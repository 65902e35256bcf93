#!/usr/bin/env python3
"""Time the fused Adam update (csrc/fused_adam.hip) on one flat fp32 bucket:

    python tools/adam_bench.py

  adam_uniform   fused_adam, uniform decay (no table)
  adam_segments  fused_adam with a ~160-segment table, decay alternating
                 1e-2 / 0 over (large, small) pairs — conv weight, BN
                 scale/shift, as no_decay_1d lays a ResNet bucket out
  fused_sgd      the momentum kernel on the same n: the streaming
                 yardstick (5 streams of 4 B per element against Adam's 7:
                 p, g, m, v in; p, m, v out)
  torch_fused    torch.optim.Adam(fused=True) over per-segment views of
                 the same flat buffers (what one would run without the
                 flat-bucket kernel)

The four alternate within each repeat. A figure is the median over repeats
of (event time of ITERS back-to-back launches) / ITERS, with min..max, in
microseconds; *_gbs is the byte model over the median. Sizes: one 25 MB
bucket (6.5M), the ResNet50_vd total (25.6M), a small 64K bucket. The
6.5M working set (4 x 26 MB) fits the 256 MB L3, so its rates can exceed
HBM's; the 25.6M one (4 x 102 MB) does not.

--rotate R gives the three HIP variants R independent buffer sets and
launch i works on set i % R, so a launch finds its operands last touched
R-1 launches ago: with R x (bytes per set) far above 256 MB every launch
starts cache-cold, as the update of a training step does after a forward
and a backward pass. torch_fused is left out of a rotated run.

    python tools/adam_bench.py --sizes 25557032 --rotate 6
    python tools/adam_bench.py --sizes 102228128     # far beyond the L3

Prints one JSON line per n."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from edl_amd.ops import ext  # noqa: E402

NSEG = 160


def time_us(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def segment_ends(n, nseg=NSEG):
    """nseg/2 (large, small) pairs filling n; small = a BN vector."""
    pairs = nseg // 2
    small = max(4, min(256, n // (8 * pairs) // 4 * 4))
    large = (n - pairs * small) // pairs // 4 * 4
    ends, off = [], 0
    for _ in range(pairs):
        off += large
        ends.append(off)
        off += small
        ends.append(off)
    ends[-1] = n
    assert all(b > a for a, b in zip([0] + ends, ends))
    return ends


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--sizes", default="6553600,25557032,65536")
    ap.add_argument("--rotate", type=int, default=1,
                    help="independent buffer sets cycled per launch")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    e = ext()
    lr, b1, b2, eps, wd, mu = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.9

    for n in (int(x) for x in args.sizes.split(",")):
        gen = torch.Generator(device="cuda").manual_seed(0)
        p, g = (torch.randn(n, device="cuda", generator=gen) for _ in range(2))
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        step = torch.ones(1, dtype=torch.int32, device="cuda")
        lr_dev = torch.full((1,), lr, device="cuda")
        ends = segment_ends(n)
        seg_end = torch.tensor(ends, dtype=torch.int32, device="cuda")
        seg_wd = torch.tensor([wd * (1 - k % 2) for k in range(len(ends))],
                              dtype=torch.float32, device="cuda")
        # torch's fused Adam over per-segment views of its own flats
        tp, tg = p.clone(), g.clone()
        views = []
        for a, b in zip([0] + ends, ends):
            t = tp[a:b].requires_grad_(True)
            t.grad = tg[a:b]
            views.append(t)
        topt = torch.optim.Adam(views, lr=lr, betas=(b1, b2), eps=eps,
                                weight_decay=wd, fused=True)

        # launch i of the HIP variants works on buffer set i % rotate
        sets = [(p, g, m, v)] + [
            (p.clone(), g.clone(), m.clone(), v.clone())
            for _ in range(args.rotate - 1)]
        turn = [0]

        def nxt():
            turn[0] += 1
            return sets[turn[0] % len(sets)]

        def adam_uniform():
            e.fused_adam(*nxt(), step, lr, b1, b2, eps, wd, 1.0, True, lr_dev)

        def adam_segments():
            e.fused_adam(*nxt(), step, lr, b1, b2, eps, 0.0, 1.0, True,
                         lr_dev, seg_end, seg_wd)

        def fused_sgd():
            sp, sg, sm, _ = nxt()
            e.fused_sgd(sp, sg, sm, lr, mu, wd, 1.0, lr_dev)

        variants = {"adam_uniform": adam_uniform,
                    "adam_segments": adam_segments, "fused_sgd": fused_sgd}
        if args.rotate == 1:
            variants["torch_fused"] = topt.step
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                samples[name].append(time_us(fn, args.iters))
        out = {"n": n, "nseg": len(ends), "iters": args.iters,
               "repeats": args.repeats, "rotate": args.rotate}
        streams = {"adam_uniform": 7, "adam_segments": 7, "fused_sgd": 5,
                   "torch_fused": 7}
        for name, s in samples.items():
            med = statistics.median(s)
            out[name + "_us"] = [round(med, 1), round(min(s), 1),
                                 round(max(s), 1)]
            out[name + "_gbs"] = round(streams[name] * 4 * n / med / 1e3, 1)
        sgd = out["fused_sgd_us"][0]
        out["adam_over_fused_sgd"] = round(out["adam_uniform_us"][0] / sgd, 2)
        out["segments_over_uniform"] = round(
            out["adam_segments_us"][0] / out["adam_uniform_us"][0], 2)
        if "torch_fused_us" in out:
            out["torch_over_adam"] = round(
                out["torch_fused_us"][0] / out["adam_uniform_us"][0], 2)
        out["model_adam_over_fused_sgd"] = round(28 / 20, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
