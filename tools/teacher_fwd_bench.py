#!/usr/bin/env python3
"""Teacher (ResNeXt101_32x16d_wsl) forward A/B: grouped-conv routing.

The distill headline (reference 656 img/s shared-GPU, README.md:84) is
bottlenecked by the teacher forward (~50 ms/bs32 on MIOpen in r1). This
sweeps EDL_CONV3X3_GROUPED_MINC — which channels-per-group widths run the
in-repo grouped implicit-GEMM kernel vs MIOpen — and checks numerics of
each variant against the all-MIOpen forward.

    python tools/teacher_fwd_bench.py [--batch 16] [--iters 10]

--eval-fuse instead A/Bs EDL_EVAL_FUSE (conv -> BN(+Add)+ReLU pairs in one
kernel, ops.conv.conv_bn): 0 and 1 interleaved in one process over --rounds
rounds, with the outputs of the two settings compared.

    python tools/teacher_fwd_bench.py --eval-fuse --iters 30 --warmup 8
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(m, x, warmup, iters):
    import torch

    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        for _ in range(warmup):
            y = m(x)
        torch.cuda.synchronize()
        t0 = time.monotonic()
        for _ in range(iters):
            y = m(x)
        torch.cuda.synchronize()
    return (time.monotonic() - t0) / iters, y


def eval_fuse_ab(args, m, x):
    """EDL_EVAL_FUSE 0 vs 1, interleaved. The fused kernels are bit-equal
    to the pairs they replace, so on a route without split-K atomics the two
    outputs are EQUAL: checked on an integer-valued input; on the randn
    input the tool's relative error is reported."""
    import torch

    import edl_amd.ops.conv as conv_mod

    assert args.rounds >= 3, "--rounds: at least three"
    xi = torch.randint(-2, 3, x.shape, device="cuda").float().contiguous(
        memory_format=torch.channels_last)
    out = {}
    for on in (False, True):
        conv_mod._EVAL_FUSE = on
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            out[on] = (m(xi).float(), m(x).float())
    equal_int = bool(torch.equal(out[False][0], out[True][0]))
    ref = out[False][1]
    d = (out[True][1] - ref).abs()
    err = float((d / ref.abs().mean().clamp(min=0.05)).max().item())
    print("integer input: outputs equal = %s; randn input: rel err = %.4g"
          % (equal_int, err), flush=True)

    ms = {False: [], True: []}
    for r in range(args.rounds):
        for on in (False, True):
            conv_mod._EVAL_FUSE = on
            dt, _ = _timed(m, x, args.warmup, args.iters)
            ms[on].append(round(dt * 1000, 3))
            print("[round %d EDL_EVAL_FUSE=%d] %7.3f ms/fwd  %8.1f img/s" %
                  (r, on, dt * 1000, args.batch / dt), flush=True)
    print(json.dumps({"bench": "teacher_fwd_eval_fuse", "model": args.model,
                      "batch": args.batch, "iters": args.iters,
                      "ms_per_fwd_unfused": ms[False],
                      "ms_per_fwd_fused": ms[True],
                      "equal_on_integer_input": equal_int,
                      "rel_err_randn": round(err, 5)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--model", default="resnext101_32x16d_wsl")
    ap.add_argument("--eval-fuse", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    import edl_amd.ops.conv as conv_mod
    from edl_amd.models import build_model

    torch.manual_seed(7)
    # same prep as distill/teacher_server.py: fp32 params, eval,
    # channels_last, bf16 autocast forward
    m = build_model(args.model).cuda()
    m = m.to(memory_format=torch.channels_last).eval()
    x = torch.randn(args.batch, 3, 224, 224, device="cuda")
    x = x.contiguous(memory_format=torch.channels_last)

    if args.eval_fuse:
        return eval_fuse_ab(args, m, x)

    results = {}
    ref = None
    for minc in (9999, 128, 64, 32, 16):
        conv_mod._GROUPED_MINC = minc
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            for _ in range(args.warmup):
                y = m(x)
            torch.cuda.synchronize()
            t0 = time.monotonic()
            for _ in range(args.iters):
                y = m(x)
            torch.cuda.synchronize()
            dt = (time.monotonic() - t0) / args.iters
        if minc == 9999:
            ref = y.float()
            err = 0.0
        else:
            d = (y.float() - ref).abs()
            err = float((d / ref.abs().mean().clamp(min=0.05)).max().item())
        results["minc%d" % minc] = {
            "ms_per_fwd": round(dt * 1000, 3),
            "img_per_s": round(args.batch / dt, 1),
            "rel_err_vs_miopen": round(err, 5),
        }
        print("[minc=%4d] %7.3f ms/fwd  %8.1f img/s  err=%.4g" %
              (minc, dt * 1000, args.batch / dt, err), flush=True)

    print(json.dumps({"bench": "teacher_fwd", "model": args.model,
                      "batch": args.batch, "results": results}))


if __name__ == "__main__":
    main()
