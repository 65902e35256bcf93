#!/usr/bin/env python3
"""Time FusedLARS.step against FusedSGD.step over the ResNet50_vd parameter
list in the reducer's flat buckets (default 25 MB cap):

    python tools/lars_bench.py

  sgd_eager / lars_eager   opt.step() launched from Python
  sgd_graph / lars_graph   one captured step, replayed
  lars_sumsq / lars_trust / lars_update
                           the three phases of a LARS step on their own
                           (eager, the optimizer's own tables)

LARS excludes the ndim <= 1 tensors (no_decay_1d), so every conv / fc
weight is reduced and owns a segment. The variants alternate within each
repeat. A figure is the median over repeats of (event time of ITERS
back-to-back steps) / ITERS, with min..max, in microseconds. Byte model per
element: SGD 20 B (p, g, m in; p, m out), LARS 28 B (p, g for the norms;
p, g, v in; p, v out), so about 1.4x plus two small launches; *_gbs is
that model over the median. The 25.6M-element working set (3 x 102 MB) is
beyond the 256 MB L3 only in part: consecutive steps find some of it
cached, as no forward/backward runs in between.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from edl_amd.models import build_model  # noqa: E402
from edl_amd.ops import ext  # noqa: E402
from edl_amd.ops.lars import FusedLARS  # noqa: E402
from edl_amd.ops.sgd import FusedSGD  # noqa: E402
from edl_amd.train.bucketed_ddp import BucketedAllReducer  # noqa: E402


def time_us(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def setup(kind, model_name, bucket_mb):
    torch.manual_seed(0)
    model = build_model(model_name, num_classes=1000).cuda()
    r = BucketedAllReducer(model.parameters(), bucket_cap_mb=bucket_mb)
    for b in r._buckets:
        b.buffer.normal_(std=1e-3)
    if kind == "sgd":
        opt = FusedSGD(model.parameters(), lr=1e-3, momentum=0.9,
                       weight_decay=1e-4, reducer=r)
    else:
        opt = FusedLARS(model.parameters(), lr=1e-3, momentum=0.9,
                        exclude=lambda p: p.ndim <= 1, reducer=r)
    opt._materialize()
    return model, r, opt


def captured(opt):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50_vd")
    ap.add_argument("--bucket_mb", type=float, default=25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    C = ext()
    _, rs, sgd = setup("sgd", args.model, args.bucket_mb)
    _, rl, lars = setup("lars", args.model, args.bucket_mb)
    n = sum(b.buffer.numel() for b in rl._buckets)
    t = lars._tables
    g0 = lars.param_groups[0]
    nchunks = t["chunks"].shape[0]

    def lars_sumsq():
        C.lars_sumsq(t["ps"], t["gs"], t["chunks"], t["bucket_off"],
                     t["partial"])

    def lars_trust():
        C.lars_trust(t["partial"], nchunks, t["tensor_chunks"], lars._trust,
                     g0["lars_coeff"], g0["lars_weight_decay"], g0["epsilon"],
                     1.0)

    def lars_update():
        for bk in lars._buckets:
            C.fused_lars(bk["p"], bk["g"], bk["v"], g0["lr"], g0["momentum"],
                         1.0, bk["seg_end"], bk["seg_wd"], bk["seg_tensor"],
                         lars._trust, lars._lr_dev)

    sgd_graph, lars_graph = captured(sgd), captured(lars)
    variants = {"sgd_eager": sgd.step, "lars_eager": lars.step,
                "sgd_graph": sgd_graph.replay, "lars_graph": lars_graph.replay,
                "lars_sumsq": lars_sumsq, "lars_trust": lars_trust,
                "lars_update": lars_update}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            samples[name].append(time_us(fn, args.iters))
    nseg = [len(bk["segs"]) for bk in lars._buckets]
    out = {"model": args.model, "n": n, "buckets": len(rl._buckets),
           "tensors": len(lars._all_params), "chunks": nchunks,
           "segments": nseg, "iters": args.iters, "repeats": args.repeats}
    streams = {"sgd_eager": 5, "sgd_graph": 5, "lars_eager": 7,
               "lars_graph": 7, "lars_sumsq": 2, "lars_update": 5}
    for name, s in samples.items():
        med = statistics.median(s)
        out[name + "_us"] = [round(med, 1), round(min(s), 1), round(max(s), 1)]
        if name in streams:
            out[name + "_gbs"] = round(streams[name] * 4 * n / med / 1e3, 1)
    for mode in ("eager", "graph"):
        out["lars_over_sgd_" + mode] = round(
            out["lars_%s_us" % mode][0] / out["sgd_%s_us" % mode][0], 2)
    out["model_lars_over_sgd"] = round(28 / 20, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
