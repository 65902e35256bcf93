"""Microbench: gemm_bt vs torch.matmul (hipBLASLt) on the ResNet50_vd
conv1x1 shapes at bs32. Run on a GPU box:
    python tools/gemm_bench.py
    python tools/gemm_bench.py --dgrad-add   # fused residual-add dgrad
    python tools/gemm_bench.py --eval-bn     # conv1x1 + eval BN in one kernel
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edl_amd import ops  # noqa: E402

# (M=N*H*W, N=Cout, K=Cin) for bs32 ResNet50_vd 1x1 convs (fwd)
SHAPES = [
    (32 * 56 * 56, 64, 64),
    (32 * 56 * 56, 256, 64),
    (32 * 56 * 56, 64, 256),
    (32 * 28 * 28, 512, 256),
    (32 * 28 * 28, 128, 512),
    (32 * 14 * 14, 1024, 512),
    (32 * 14 * 14, 256, 1024),
    (32 * 7 * 7, 2048, 1024),
    (32 * 7 * 7, 512, 2048),
]


def bench(fn, iters=30, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.monotonic()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.monotonic() - t0) / iters


def main():
    print("%-28s %10s %10s %8s" % ("shape (M,N,K)", "gemm_bt", "hipBLASLt", "ratio"))
    for M, N, K in SHAPES:
        a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
        b = torch.randn(N, K, device="cuda").to(torch.bfloat16)
        flops = 2.0 * M * N * K
        t_hip = bench(lambda: ops.ext().gemm_bt(a, b))
        bt = b.t().contiguous()
        t_blas = bench(lambda: a @ b.t())
        print("%-28s %7.1f TF %7.1f TF %7.2fx" % (
            str((M, N, K)), flops / t_hip / 1e12, flops / t_blas / 1e12,
            t_blas / t_hip))


def main_wgrad():
    """Wgrad: direct TN kernel vs the transpose_pad + bt_splitk pipeline.
    Shapes are the ResNet50_vd 1x1 wgrads at bs32: C[Cout,Cin] over K=M."""
    e = ops.ext()
    print("%-28s %10s %10s %8s" % ("shape (K,N1,N2)", "tn", "pad+bt", "ratio"))
    for M, Cout, Cin in SHAPES:
        a = torch.randn(M, Cout, device="cuda").to(torch.bfloat16)
        b = torch.randn(M, Cin, device="cuda").to(torch.bfloat16)
        flops = 2.0 * M * Cout * Cin
        t_tn = bench(lambda: e.gemm_tn_splitk(a, b, 0))
        t_bt = bench(lambda: e.gemm_bt_splitk(
            e.transpose_pad(a), e.transpose_pad(b), 0))
        print("%-28s %7.1f TF %7.1f TF %7.2fx" % (
            str((M, Cout, Cin)), flops / t_tn / 1e12, flops / t_bt / 1e12,
            t_bt / t_tn))


def main_wgrad3():
    """conv3x3 wgrad: direct TN gather vs transpose_pad+shift9+bt.
    (N, Cin, H, W, Cout, stride) = bs32 ResNet50_vd 3x3 convs."""
    e = ops.ext()
    shapes = [
        (32, 64, 56, 56, 64, 1),
        (32, 128, 28, 28, 128, 1), (32, 128, 56, 56, 128, 2),
        (32, 256, 14, 14, 256, 1), (32, 256, 28, 28, 256, 2),
        (32, 512, 7, 7, 512, 1), (32, 512, 14, 14, 512, 2),
    ]
    print("%-28s %10s %10s %8s" % ("(N,C,H,W,s)", "tn3x3", "old", "ratio"))
    for n, ci, h, w, co, s in shapes:
        x = torch.randn(n, ci, h, w, device="cuda").to(torch.bfloat16)
        x = x.contiguous(memory_format=torch.channels_last)
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        dy = torch.randn(n * ho * wo, co, device="cuda").to(torch.bfloat16)
        flops = 2.0 * n * ho * wo * co * 9 * ci
        t_tn = bench(lambda: e.gemm_tn3x3_splitk(dy, x, s, 0))
        t_bt = bench(lambda: e.gemm_bt_splitk(
            e.transpose_pad(dy), e.conv3x3_wgrad_operand(x, s), 0))
        print("%-28s %7.1f TF %7.1f TF %7.2fx" % (
            str((n, ci, h, w, s)), flops / t_tn / 1e12, flops / t_bt / 1e12,
            t_bt / t_tn))


def _graph_us(fn, sets, windows):
    """Sorted us per call of fn(*set) over `windows` event-timed replays of
    one graph-captured pass over the operand sets."""
    for ops_ in sets:  # warm-up pass
        fn(*ops_)
    torch.cuda.synchronize()
    # one pass over the sets as a graph: the step runs captured, so host
    # launch cost must not count against a two-kernel variant
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for ops_ in sets:
            fn(*ops_)
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(windows):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        g.replay()
        t1.record()
        torch.cuda.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / len(sets))
    del g
    return sorted(us)


# (M, N=Cin, K=Cout, blocks) of the 16 BottleneckVd conv0 dgrads at bs32
DGRAD_ADD_SHAPES = [
    (100352, 64, 64, 1), (100352, 256, 64, 2), (100352, 256, 128, 1),
    (25088, 512, 128, 3), (25088, 512, 256, 1),
    (6272, 1024, 256, 5), (6272, 1024, 512, 1),
    (1568, 2048, 512, 2),
]


def main_dgrad_add(windows=9, l3_bytes=256 << 20):
    """conv0 dgrad + residual-gradient add, per shape: (a) gemm_bt + torch
    add, (b) gemm_bt_add, (c) gemm_bt alone. Operands rotate over enough
    buffer sets to exceed the L3, as the training step sees them cold.
    Median [min..max] us per call over `windows` event-timed replays of one
    graph-captured pass over the sets. EDL_BT_ADD_R=global selects the other R-load
    variant of (b): run once per variant."""
    e = ops.ext()
    print("R load: %s" % os.environ.get("EDL_BT_ADD_R", "lds"))
    print("%-22s %3s %-24s %-24s %-24s" % (
        "shape (M,N,K)", "x", "(a) bt + add", "(b) bt_add", "(c) bt alone"))
    tot = {"a": 0.0, "b": 0.0, "c": 0.0}
    for M, N, K, cnt in DGRAD_ADD_SHAPES:
        set_bytes = 2 * (M * K + N * K + 2 * M * N)
        nsets = max(2, -(-int(1.25 * l3_bytes) // set_bytes))
        sets = [(torch.randn(M, K, device="cuda").to(torch.bfloat16),
                 torch.randn(N, K, device="cuda").to(torch.bfloat16),
                 torch.randn(M, N, device="cuda").to(torch.bfloat16))
                for _ in range(nsets)]
        fns = {
            "a": lambda a, b, r: e.gemm_bt(a, b) + r,
            "b": lambda a, b, r: e.gemm_bt_add(a, b, r),
            "c": lambda a, b, r: e.gemm_bt(a, b),
        }
        cols = []
        for key in ("a", "b", "c"):
            us = _graph_us(fns[key], sets, windows)
            med = us[len(us) // 2]
            tot[key] += med * cnt
            cols.append("%7.1f [%6.1f..%6.1f]" % (med, us[0], us[-1]))
        print("%-22s %3d %-24s %-24s %-24s" % (str((M, N, K)), cnt, *cols))
        del sets
        torch.cuda.empty_cache()
    print("per step (x counts): (a) %.1f us  (b) %.1f us  (c) %.1f us" % (
        tot["a"], tot["b"], tot["c"]))


def _bottleneck_1x1_shapes(batch, stem_c, planes, depths, width_of):
    """Distinct 1x1 GEMMs of a bottleneck net's forward at 224 px, as
    {(M, N, K, residual, relu): count}: per block the reduce conv (ReLU), the
    expand conv (+ shortcut, ReLU) and, in a stage's first block, the
    projection shortcut (plain BN). The stride sits on the 3x3, so a first
    block's reduce conv still runs at the previous stage's extent."""
    out = {}

    def add(*key):
        out[key] = out.get(key, 0) + 1

    cin, hw = stem_c, 56
    for si, (p, d) in enumerate(zip(planes, depths)):
        hw_in, hw = hw, hw if si == 0 else hw // 2
        w, cout = width_of(p), 4 * p
        for i in range(d):
            m_in = batch * (hw_in if i == 0 else hw) ** 2
            m = batch * hw * hw
            add(m_in, w, cin, False, True)
            add(m, cout, w, True, True)
            if i == 0:
                add(m, cout, cin, False, False)
            cin = cout
    return out


def main_eval_bn(windows=9, l3_bytes=256 << 20):
    """conv1x1 -> eval BN(+Add)+ReLU per shape, with and without a residual:
    (a) gemm_bt + bn_fwd_eval (two launches), (b) gemm_bt_bn, (c) gemm_bt
    alone. Cold operands and timing as --dgrad-add. `x` is how often the
    forward runs that form (0: the other form of a shape, timed for
    comparison, not in the totals). `fused` is what ops.conv.conv_bn does
    with the shape by default: BNs wider than 2048 keep their own launch."""
    e = ops.ext()
    nets = [
        ("ResNeXt101_32x16d bs16", _bottleneck_1x1_shapes(
            16, 64, (64, 128, 256, 512), (3, 4, 23, 3), lambda p: 8 * p)),
        ("ResNet50_vd bs32", _bottleneck_1x1_shapes(
            32, 64, (64, 128, 256, 512), (3, 4, 6, 3), lambda p: p)),
    ]
    for name, shapes in nets:
        for M, N, K, res, relu in list(shapes):
            if not any(k[:4] == (M, N, K, not res) for k in shapes):
                shapes[(M, N, K, not res, relu)] = 0
        print(name)
        print("%-22s %3s %3s %4s %-24s %-24s %-24s %s" % (
            "shape (M,N,K)", "res", "act", "x", "(a) bt + bn_apply",
            "(b) bt_bn", "(c) bt alone", "fused"))
        tot = {"a": 0.0, "b": 0.0, "c": 0.0}
        for (M, N, K, res, relu), cnt in sorted(
                shapes.items(), key=lambda kv: (-kv[0][0], kv[0][1:])):
            set_bytes = 2 * (M * K + N * K + (3 if res else 2) * M * N)
            nsets = max(2, -(-int(1.25 * l3_bytes) // set_bytes))
            sets = [(torch.randn(M, K, device="cuda").to(torch.bfloat16),
                     torch.randn(N, K, device="cuda").to(torch.bfloat16),
                     torch.randn(M, N, device="cuda").to(torch.bfloat16)
                     if res else None,
                     torch.randn(N, device="cuda"),
                     torch.randn(N, device="cuda"))
                    for _ in range(nsets)]
            fns = {
                "a": lambda a, b, r, sc, sh: e.bn_fwd_eval(
                    e.gemm_bt(a, b), sc, sh, r, relu),
                "b": lambda a, b, r, sc, sh: e.gemm_bt_bn(
                    a, b, sc, sh, relu, r),
                "c": lambda a, b, r, sc, sh: e.gemm_bt(a, b),
            }
            cols = []
            for key in ("a", "b", "c"):
                us = _graph_us(fns[key], sets, windows)
                med = us[len(us) // 2]
                tot[key] += med * cnt
                cols.append("%7.1f [%6.1f..%6.1f]" % (med, us[0], us[-1]))
            print("%-22s %3s %3s %4d %-24s %-24s %-24s %s" % (
                str((M, N, K)), "+R" if res else "-", "y" if relu else "n",
                cnt, *cols, "yes" if N <= 2048 else "no (wide BN)"),
                flush=True)
            del sets
            torch.cuda.empty_cache()
        print("per forward (x counts): (a) %.1f us  (b) %.1f us  (c) %.1f us"
              % (tot["a"], tot["b"], tot["c"]))


if __name__ == "__main__":
    if "--dgrad-add" in sys.argv:
        main_dgrad_add()
    elif "--eval-bn" in sys.argv:
        main_eval_bn()
    elif "--wgrad" in sys.argv:
        main_wgrad()
    elif "--wgrad3" in sys.argv:
        main_wgrad3()
    else:
        main()
