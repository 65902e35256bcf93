"""Microbench: training BatchNorm+ReLU at C = 4096 (stage 4 of
ResNeXt101_32x16d at batch 16 and 32), forward and forward+backward:
  (a) BNReLU2d._fallback under autograd (fp32 copy, library BN, ReLU, cast):
      the route these widths took before bn_wide.hip;
  (b) the bn_wide kernels as the launcher picks slab width and variant;
  (c) forced to the other slab width, W = 64 (EDL_BN_WIDE_W);
  (d) forced to the streaming variant (EDL_BN_WIDE_RESIDENT=0) where (b)
      keeps the slab resident in LDS ("-" where (b) streams already).
Run on a GPU box, with a time limit on the command:
    timeout 600 python tools/bn_wide_bench.py
Median [min..max] us per call over 9 event-timed replays of one
graph-captured pass over operand sets that rotate past the 256 MB L3; the
columns of a row are captured once each and replayed in turn, as
tools/gemm_bench.py --stem7-wgrad does. MB: what a pass has to move at the
least (fwd: x in, y and the mask out; f+b adds dy, x and the mask in, dx
out); GB/s: that over the median of (b)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edl_amd import ops  # noqa: E402
from edl_amd.ops.bnrelu import BNReLU2d  # noqa: E402
from gemm_bench import _graph_us_alternating  # noqa: E402

# (N, C, H, W): M = N*H*W = 784, 3136, 1568, 6272
SHAPES = [(16, 4096, 7, 7), (16, 4096, 14, 14), (32, 4096, 7, 7),
          (32, 4096, 14, 14)]
SWITCHES = ("EDL_BN_WIDE_W", "EDL_BN_WIDE_RESIDENT")


def _route(env, backward):
    """fn(m, x, dy) that runs one BN under the launcher switches in env
    (None: the torch fallback). The launchers read them per call, so they
    only need to be set while the call is made or captured."""
    def f(m, x, dy):
        if env is None:
            y = m._fallback(x)
        else:
            os.environ.update(env)
            y = m(x)
        if backward:
            y.backward(dy)
        for k in SWITCHES:
            os.environ.pop(k, None)
    return f


def main(windows=9, l3_bytes=256 << 20):
    assert torch.cuda.is_available(), "bn_wide_bench needs a GPU"
    for k in SWITCHES:
        os.environ.pop(k, None)
    e = ops.ext()
    print("%-20s %-4s %7s %-24s %-24s %-24s %-24s %6s %7s" % (
        "shape (N,C,H,W)", "pass", "MB", "(a) fallback", "(b) bn_wide",
        "(c) other W", "(d) streaming", "a/b", "GB/s(b)"))
    for N, C, H, W in SHAPES:
        M = N * H * W
        set_bytes = 2 * 2 * M * C
        nsets = max(2, -(-int(1.25 * l3_bytes) // set_bytes))
        sets = []
        for _ in range(nsets):
            x = torch.randn(N, C, H, W, device="cuda").to(torch.bfloat16)
            x = x.contiguous(memory_format=torch.channels_last)
            dy = torch.randn(N, C, H, W, device="cuda").to(torch.bfloat16)
            dy = dy.contiguous(memory_format=torch.channels_last)
            sets.append((BNReLU2d(C).cuda().train(), x.requires_grad_(True),
                         dy))
        for name, backward in (("fwd", 0), ("f+b", 1)):
            # the launcher's own picks, read with no switch set
            resident = M <= e.bn_wide_resident_rows(C, backward) and (
                not backward or M <= e.bn_wide_resident_rows(C, 0))
            fns = {"a": _route(None, backward), "b": _route({}, backward),
                   "c": _route({"EDL_BN_WIDE_W": "64"},
                               backward)}
            if resident:
                fns["d"] = _route({"EDL_BN_WIDE_RESIDENT": "0"}, backward)
            us = _graph_us_alternating(fns, sets, windows)
            mb = 4 * M * C + M * C // 8 + backward * (6 * M * C + M * C // 8)
            cols = ["%7.1f [%6.1f..%6.1f]" % (v[len(v) // 2], v[0], v[-1])
                    if v else "-" for v in (us.get(k) for k in "abcd")]
            med = {k: v[len(v) // 2] for k, v in us.items()}
            print("%-20s %-4s %7.1f %-24s %-24s %-24s %-24s %5.2fx %7.0f" % (
                str((N, C, H, W)), name, mb / 1e6, *cols, med["a"] / med["b"],
                mb / med["b"] / 1e3), flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
