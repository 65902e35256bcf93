#!/usr/bin/env python3
"""Time the DGC compress chain (csrc/dgc.hip: accumulate, pick, hist,
pick, hist, pick, compact) against the chain it replaces, written as in
DGCCompressor.step (add_, abs, topk, gather, indexed zero), on one flat
fp32 bucket of randn data at sparsity 0.999.

    python tools/dgc_bench.py

The two chains alternate within each repeat; u, v (and the residual) are
restored from saved copies before each timed block so every repeat sees
the same data. A figure is the median over repeats of (event time of
ITERS back-to-back iterations) / ITERS, with min..max. fused_sgd on the
same n is the streaming yardstick (5 streams of 4 B per element). The
per-kernel rows time each kernel back-to-back on its own: hist1 / hist2
filter on the prefix a real step gives them; dgc_compact runs on the
step's v and threshold with the cursor already spent, so it does the
read, the ballots, the staging and the cursor claims of a real step, but
its `slot < k` guard drops the scattered writes (0.1% of the elements).
A kernel trace of the chain itself (rocprofv3 --kernel-trace --stats)
gives the in-sequence durations. Prints one JSON line per n."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from edl_amd.ops import ext  # noqa: E402


def time_us(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--sizes", default="6553600,25557032")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    e = ext()
    mu, wd, lr = 0.9, 1e-4, 0.1

    for n in (int(x) for x in args.sizes.split(",")):
        k = max(1, int(n * (1 - 0.999)))
        gen = torch.Generator(device="cuda").manual_seed(0)
        g, u0, v0, p = (torch.randn(n, device="cuda", generator=gen)
                        for _ in range(4))
        u, v, res = u0.clone(), v0.clone(), v0.clone()
        m = torch.zeros_like(p)
        ws = torch.zeros(e.dgc_workspace_words(), dtype=torch.int32,
                         device="cuda")
        ws_scratch = ws.clone()  # for the kernels timed out of sequence
        payload = torch.empty(2, k, dtype=torch.int32, device="cuda")

        def restore():
            u.copy_(u0)
            v.copy_(v0)
            res.copy_(v0)

        def hip_chain(copies=4):
            e.dgc_accumulate(g, u, v, p, mu, wd, ws, copies)
            e.dgc_select(v, u, payload, ws)

        def torch_chain():
            res.add_(g)
            _, idx = torch.topk(res.abs(), k, sorted=False)
            vals = res[idx].clone()
            res[idx] = 0
            return idx, vals

        kernels = {
            "accumulate_1copy": lambda: e.dgc_accumulate(
                g, u, v, p, mu, wd, ws_scratch, 1),
            "accumulate_4copy": lambda: e.dgc_accumulate(
                g, u, v, p, mu, wd, ws_scratch, 4),
            "accumulate_4copy_no_p": lambda: e.dgc_accumulate(
                g, u, v, None, mu, 0.0, ws_scratch, 4),
            "pick0": lambda: e.dgc_pick(v, ws_scratch, 0, k),
            "hist1": lambda: e.dgc_hist(v, ws_scratch, 1),
            "hist2": lambda: e.dgc_hist(v, ws_scratch, 2),
            "compact": lambda: e.dgc_compact(v, u, payload, ws),
            "fused_sgd": lambda: e.fused_sgd(p, g, m, lr, mu, wd, 1.0, None),
        }
        chains = {"hip": hip_chain, "hip_1copy": lambda: hip_chain(1),
                  "torch": torch_chain}
        for fn in list(chains.values()) + list(kernels.values()):
            restore()
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # the selection itself, once, on the restored data
        restore()
        hip_chain()
        nsel = int((payload[0] >= 0).sum())

        samples = {name: [] for name in list(chains) + list(kernels)}
        for _ in range(args.repeats):
            for name, fn in chains.items():
                restore()
                samples[name].append(time_us(fn, args.iters))
            for name, fn in kernels.items():
                if name in ("hist1", "hist2"):
                    # the prefix this pass filters on in a real step
                    restore()
                    ws_scratch.zero_()
                    e.dgc_accumulate(g, u, v, p, mu, wd, ws_scratch, 4)
                    e.dgc_pick(v, ws_scratch, 0, k)
                    if name == "hist2":
                        e.dgc_hist(v, ws_scratch, 1)
                        e.dgc_pick(v, ws_scratch, 1, k)
                elif name == "compact":
                    restore()
                    hip_chain()  # leaves the threshold (and a spent cursor)
                    restore()
                    e.dgc_accumulate(g, u, v, p, mu, wd, ws_scratch, 4)
                samples[name].append(time_us(fn, args.iters))
        out = {"n": n, "k": k, "nsel": nsel, "iters": args.iters,
               "repeats": args.repeats}
        for name, s in samples.items():
            out[name + "_us"] = [round(statistics.median(s), 1),
                                 round(min(s), 1), round(max(s), 1)]
        sgd = out["fused_sgd_us"][0]
        out["hip_over_fused_sgd"] = round(out["hip_us"][0] / sgd, 2)
        out["torch_over_hip"] = round(out["torch_us"][0] / out["hip_us"][0], 2)
        # bytes model: accumulate 6 streams with p (g, u, v, p in; u, v
        # out), 1 stream for each of hist1, hist2, compact; fused_sgd 5
        out["model_streams_hip"] = 9
        out["model_hip_over_fused_sgd"] = round(9 / 5, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
