#!/usr/bin/env python3
"""Time the image input kernel (csrc/image_prep.hip) on one training batch:
B decoded 500x375 sources, each with a seeded random-area/aspect window and
a mirror coin (data/images.py draw_train_window), packed as the loader packs
them, resampled to S x S:

    python tools/image_prep_bench.py

  hip_bf16    the kernel, channels-last bf16 out (what the trainer runs)
  hip_fp32    the kernel, channels-last fp32 out
  op_bf16     hip_bf16 through ops.image_prep.crop_resize_normalize with a
              pinned host table: the host check of the table and its upload
              on top of the launch
  torch       the same batch in torch ops on the same GPU: per image, crop
              -> F.interpolate(bilinear) -> flip -> normalize, then stack and
              convert to channels-last bf16
  h2d_fp32    the upload the synthetic loader does per step: one pinned fp32
              [B, 3, S, S] batch, host to device
  h2d_u8      the upload this path does instead: the packed uint8 windows

The variants alternate within each repeat. A figure is the median over
repeats of (event time of ITERS back-to-back launches) / ITERS, with
min..max, in microseconds. The byte model of the kernel is its output
(3 * itemsize per pixel) plus the packed bytes read once; *_gbs is that over
the median.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from edl_amd.data.images import draw_train_window  # noqa: E402
from edl_amd.ops import ext  # noqa: E402
from edl_amd.ops.image_prep import (IMAGENET_MEAN, IMAGENET_STD,  # noqa: E402
                                    crop_resize_normalize, make_table)


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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--src_hw", default="375x500")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    C = ext()
    B, S = args.batch, args.size
    H, W = (int(v) for v in args.src_hw.split("x"))
    dev = torch.device("cuda")

    rng = np.random.RandomState(0)
    gen = torch.Generator().manual_seed(0)
    chunks, rows, wins, off = [], [], [], 0
    for _ in range(B):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        x0, y0, cw, ch, flip = draw_train_window(H, W, gen)
        xh, yh = min(W, x0 + cw + 1), min(H, y0 + ch + 1)
        crop = np.ascontiguousarray(img[y0:yh, x0:xh])
        rows.append((off, crop.shape[0], crop.shape[1], flip, 0, 0, cw, ch))
        wins.append((cw, ch, flip))
        chunks.append(crop.reshape(-1))
        off += crop.size
    host_packed = torch.from_numpy(np.concatenate(chunks)).pin_memory()
    host_table = make_table(rows).pin_memory()
    packed = host_packed.to(dev)
    table = host_table.to(dev)
    mean, std = list(IMAGENET_MEAN), list(IMAGENET_STD)
    crops = [packed[r[0]:r[0] + 3 * r[1] * r[2]].view(r[1], r[2], 3)
             for r in rows]
    mean_t = torch.tensor(mean, device=dev).view(1, 3, 1, 1) * 255.0
    istd_t = 1.0 / (torch.tensor(std, device=dev).view(1, 3, 1, 1) * 255.0)
    host_f32 = torch.randn(B, 3, S, S).pin_memory()
    dev_f32 = torch.empty(B, 3, S, S, device=dev)
    dev_u8 = torch.empty_like(packed)

    def hip_bf16():
        C.crop_resize_normalize(packed, table, S, mean, std, True)

    def hip_fp32():
        C.crop_resize_normalize(packed, table, S, mean, std, False)

    def op_bf16():
        crop_resize_normalize(packed, host_table, S, mean, std, torch.bfloat16)

    def torch_path():
        outs = []
        for img, (cw, ch, flip) in zip(crops, wins):
            x = img[:ch, :cw].permute(2, 0, 1)[None].float()
            x = F.interpolate(x, (S, S), mode="bilinear", align_corners=False,
                              antialias=False)
            if flip:
                x = x.flip(3)
            outs.append((x - mean_t) * istd_t)
        return torch.cat(outs).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last)

    def h2d_fp32():
        dev_f32.copy_(host_f32, non_blocking=True)

    def h2d_u8():
        dev_u8.copy_(host_packed, non_blocking=True)

    # the two paths agree before either is timed
    a = C.crop_resize_normalize(packed, table, S, mean, std, False)
    b = torch_path().float()
    agree = float((a - b).abs().max())

    variants = {"hip_bf16": hip_bf16, "hip_fp32": hip_fp32,
                "op_bf16": op_bf16, "torch": torch_path,
                "h2d_fp32": h2d_fp32, "h2d_u8": h2d_u8}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            samples[name].append(time_us(fn, args.iters))
    nbytes = packed.numel()
    out = {"batch": B, "size": S, "src_hw": [H, W], "packed_bytes": nbytes,
           "iters": args.iters, "repeats": args.repeats,
           "hip_vs_torch_max_abs": round(agree, 4)}
    model = {"hip_bf16": B * S * S * 6 + nbytes,
             "hip_fp32": B * S * S * 12 + nbytes,
             "h2d_fp32": B * S * S * 12, "h2d_u8": nbytes}
    for name, s in samples.items():
        med = statistics.median(s)
        out[name + "_us"] = [round(med, 1), round(min(s), 1),
                             round(max(s), 1)]
        if name in model:
            out[name + "_bytes"] = model[name]
            out[name + "_gbs"] = round(model[name] / med / 1e3, 1)
    out["torch_over_hip_bf16"] = round(
        out["torch_us"][0] / out["hip_bf16_us"][0], 2)
    out["h2d_fp32_over_h2d_u8"] = round(
        out["h2d_fp32_us"][0] / out["h2d_u8_us"][0], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
