#!/usr/bin/env python3
"""BN backward microbench per ResNet50_vd batch-32 layer class, row-only
partition of the reduce (EDL_BN_SLAB=0) against the channel-slab one
(EDL_BN_SLAB=1), alternating in one process.

Per class and setting, median [min..max] us of 9 event-timed replays of one
graph-captured pass over operand sets that together exceed the 256 MB L3
(tools/gemm_bench.py, _graph_us_alternating):
  whole   bn_bwd(training=True): reduce + finalize + dx
  frozen  bn_bwd(training=False): the same reduce + finalize, and a dx that
          reads dy and the mask only
The two settings differ in the reduce (and the partial rows the finalize
reads) alone, so old - new of either column is what the reduce gained. No
binding runs the reduce by itself: its own time comes from a kernel trace
of bench.py (profiles/bn_reduce_slab_trace_before_after.txt). GB/s here is the reduce's
4.125 B/element (dy, x, one mask byte per octet) over the FROZEN call, a
lower bound of the reduce's rate.

    python tools/bn_bwd_bench.py [--windows 9]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# (M, C, relu, add, calls per backward) of the 55 BN outputs
SHAPES = [
    (32 * 112 * 112, 32, True, False, 2),    # stem conv0/conv1
    (32 * 112 * 112, 64, True, False, 1),    # stem conv2
    (32 * 56 * 56, 64, True, False, 6),      # stage1 1x1/3x3
    (32 * 56 * 56, 128, True, False, 1),     # stage2 block0 conv0
    (32 * 56 * 56, 256, True, True, 3),      # stage1 tails
    (32 * 56 * 56, 256, False, False, 1),    # stage1 projection
    (32 * 28 * 28, 128, True, False, 7),
    (32 * 28 * 28, 256, True, False, 1),     # stage3 block0 conv0
    (32 * 28 * 28, 512, True, True, 4),
    (32 * 28 * 28, 512, False, False, 1),
    (32 * 14 * 14, 256, True, False, 11),
    (32 * 14 * 14, 512, True, False, 1),     # stage4 block0 conv0
    (32 * 14 * 14, 1024, True, True, 6),
    (32 * 14 * 14, 1024, False, False, 1),
    (32 * 7 * 7, 512, True, False, 5),
    (32 * 7 * 7, 2048, True, True, 3),
    (32 * 7 * 7, 2048, False, False, 1),
]
assert sum(s[4] for s in SHAPES) == 55

L3_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--max-sets", type=int, default=64)
    args = ap.parse_args()

    import torch

    from edl_amd import ops
    from gemm_bench import _graph_us_alternating

    assert torch.cuda.is_available(), "bn_bwd_bench needs an MI355X"
    e = ops.ext()
    torch.manual_seed(3)

    def call(slab, training, relu, add):
        def fn(dy, mask, x, mean, invstd, gamma):
            os.environ["EDL_BN_SLAB"] = slab  # read per call by bn_bwd
            e.bn_bwd(dy, mask, x, mean, invstd, gamma, relu, add, training,
                     None, None)
        return fn

    keys = [("whole", "0"), ("whole", "1"), ("frozen", "0"), ("frozen", "1")]
    print("%-26s %2s  %-24s %-24s %-24s %-24s %9s %9s" % (
        "(M, C, relu, add)", "x", "whole SLAB=0", "whole SLAB=1",
        "frozen SLAB=0", "frozen SLAB=1", "GB/s 0", "GB/s 1"))
    tot = {k: 0.0 for k in keys}
    slower = []
    for (M, C, relu, add, w) in SHAPES:
        set_bytes = int(M * C * 4.125)
        nsets = min(args.max_sets,
                    max(2, -(-int(1.25 * L3_BYTES) // set_bytes)))
        sets = [(torch.randn(M, C, device="cuda").to(torch.bfloat16),
                 torch.randint(0, 256, (M, C // 8), device="cuda",
                               dtype=torch.uint8) if relu else None,
                 torch.randn(M, C, device="cuda").to(torch.bfloat16),
                 torch.randn(C, device="cuda") * 0.1,
                 torch.rand(C, device="cuda") + 0.5,
                 torch.ones(C, device="cuda"))
                for _ in range(nsets)]
        fns = {(kind, slab): call(slab, kind == "whole", relu, add)
               for kind, slab in keys}
        us = _graph_us_alternating(fns, sets, args.windows)
        med = {k: u[len(u) // 2] for k, u in us.items()}
        for k in keys:
            tot[k] += med[k] * w
        cols = ["%7.1f [%6.1f..%6.1f]" % (med[k], us[k][0], us[k][-1])
                for k in keys]
        gbs = [set_bytes / med[("frozen", s)] / 1e3 for s in ("0", "1")]
        print("%-26s %2d  %-24s %-24s %-24s %-24s %9.0f %9.0f" % (
            str((M, C, int(relu), int(add))), w, *cols, *gbs), flush=True)
        # slower than the row-only partition by more than both spreads
        o, n = us[("whole", "0")], us[("whole", "1")]
        if n[len(n) // 2] - o[len(o) // 2] > (o[-1] - o[0]) + (n[-1] - n[0]):
            slower.append((M, C, relu, add))
        del sets
        torch.cuda.empty_cache()
    os.environ.pop("EDL_BN_SLAB", None)
    print("classes slower under EDL_BN_SLAB=1 by more than the two spreads: %s"
          % (slower or "none"))
    print(json.dumps({"bench": "bn_bwd", "us_per_step": {
        "%s_slab%s" % k: round(v, 1) for k, v in tot.items()}}))


if __name__ == "__main__":
    main()
