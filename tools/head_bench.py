"""Microbench: the classifier head, (a) torch under bf16 autocast
(adaptive_avg_pool2d + nn.Linear: mean reduce, weight cast, hipBLASLt GEMMs)
against (b) ops.head.pool_linear (csrc/head.hip), forward and
forward+backward. Run on a GPU box:
    python tools/head_bench.py
Median [min..max] us per call over 9 event-timed replays of one
graph-captured pass over operand sets that rotate past the 256 MB L3, as
tools/gemm_bench.py --dgrad-add does. (b) reads a bf16 weight cached on the
module, which is what the engine's bf16 mirror gives it in training."""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edl_amd.ops import head  # noqa: E402
from gemm_bench import _graph_us  # noqa: E402

# (N, C, H, W, K)
SHAPES = [(32, 2048, 7, 7, 1000), (16, 2048, 7, 7, 1000),
          (32, 512, 7, 7, 1000), (256, 2048, 7, 7, 1000)]


def _torch_head(x, fc):
    return fc(F.adaptive_avg_pool2d(x, 1).flatten(1))


def _fwd(route):
    def f(x, fc, dl):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return route(x, fc)
    return f


def _fwd_bwd(route):
    def f(x, fc, dl):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = route(x, fc)
        y.backward(dl)
    return f


def main(windows=9, l3_bytes=256 << 20):
    assert torch.cuda.is_available(), "head_bench needs a GPU"
    # time the kernels on every shape, also where pool_linear's routing
    # rule would hand the batch to torch (that is how the rule was found)
    head._MAX_ROUTE_ROWS = head._MAX_ROWS
    print("%-26s %-4s %-26s %-26s %6s" % (
        "shape (N,C,H,W,K)", "pass", "(a) torch autocast", "(b) pool_linear",
        "a/b"))
    for N, C, H, W, K in SHAPES:
        set_bytes = 2 * 2 * N * C * H * W + 2 * 4 * K * C
        nsets = max(2, -(-int(1.25 * l3_bytes) // set_bytes))
        sets = []
        for _ in range(nsets):
            x = torch.randn(N, C, H, W, device="cuda").to(torch.bfloat16)
            x = x.contiguous(memory_format=torch.channels_last)
            sets.append((x.requires_grad_(True), nn.Linear(C, K).cuda(),
                         torch.randn(N, K, device="cuda").to(torch.bfloat16)))
        for name, wrap in (("fwd", _fwd), ("f+b", _fwd_bwd)):
            cols, med = [], []
            for route in (_torch_head, head.pool_linear):
                us = _graph_us(wrap(route), sets, windows)
                med.append(us[len(us) // 2])
                cols.append("%7.1f [%6.1f..%6.1f]" % (med[-1], us[0], us[-1]))
            print("%-26s %-4s %-26s %-26s %5.2fx" % (
                str((N, C, H, W, K)), name, *cols, med[0] / med[1]),
                flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
