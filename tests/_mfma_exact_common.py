"""Integer-exact checking of the MFMA kernels (gemm_bt, gemm_tn, conv3x3).

bf16 holds small integers exactly and an MFMA product of two of them is
exact; every partial sum whose magnitude stays below 2^24 is exact in fp32
in ANY order (K-loop order, KW folds in LDS, split-K atomics in arrival
order). On such operands an fp32 output is bit-equal to the fp64 reference
and a bf16 output is bit-equal to the reference rounded once to bf16 — so a
dropped or doubled K element, a tail row clamped into the wrong place or a
split-K slice folded twice moves the result instead of hiding in a
tolerance. What the idiom cannot see is rounding INSIDE the accumulator
(integers never round there); a real-valued case with a derived bound
covers that separately.

Everything here computes its references in fp64 on the CPU, whatever
device the operands live on, and runs without a GPU.
"""
import torch
import torch.nn.functional as F

TWO24 = float(1 << 24)

# value sets: all non-zero (a zero would hide a dropped term); the operands
# of one product are drawn independently and from different sets, so a
# swapped row, column or k index changes the sum
PM1 = (-1, 1)
PM12 = (-2, -1, 1, 2)
ASYM3 = (-3, -1, 2, 3)


def ints(shape, values, gen):
    """bf16 CPU tensor drawn uniformly from `values` (non-zero integers)."""
    assert len(values) >= 2
    for v in values:
        assert int(v) == v and v != 0 and abs(v) <= 256, values
    table = torch.tensor(values, dtype=torch.float32)
    idx = torch.randint(len(values), tuple(shape), generator=gen)
    return table[idx].to(torch.bfloat16)


def _d(t):
    return t.detach().to("cpu", torch.float64)


def exact_ref_bt(a, b):
    """fp64 A[M,K] @ B[N,K]^T."""
    return _d(a) @ _d(b).t()


def exact_ref_tn(a, b):
    """fp64 A[K,N1]^T @ B[K,N2]."""
    return _d(a).t() @ _d(b)


def exact_ref_conv(x, w, stride, groups=1):
    """fp64 3x3 pad-1 conv as unfold + matmul: x [N,Cin,H,W], w
    [Cout,Cin/groups,3,3] -> [N,Cout,Ho,Wo]."""
    xd, wd = _d(x).contiguous(), _d(w)
    n, cin, h, wi = xd.shape
    cout, cpg = wd.shape[0], wd.shape[1]
    assert cin == cpg * groups and cout % groups == 0
    ho, wo = (h - 1) // stride + 1, (wi - 1) // stride + 1
    cols = F.unfold(xd, 3, padding=1, stride=stride)      # [N, Cin*9, L]
    cols = cols.view(n, groups, cpg * 9, ho * wo)
    wm = wd.reshape(groups, cout // groups, cpg * 9)
    y = torch.einsum("gok,ngkl->ngol", wm, cols)
    return y.reshape(n, cout, ho, wo)


def exact_ref_conv_dx(x_shape, w, dy, stride):
    """fp64 input gradient of the 3x3 pad-1 conv -> [N,Cin,H,W]."""
    return torch.nn.grad.conv2d_input(
        list(x_shape), _d(w), _d(dy).contiguous(), stride=(stride, stride),
        padding=(1, 1))


def exact_ref_conv_dw(x, w_shape, dy, stride):
    """fp64 weight gradient of the 3x3 pad-1 conv -> [Cout,Cin,3,3]."""
    return torch.nn.grad.conv2d_weight(
        _d(x).contiguous(), tuple(w_shape), _d(dy).contiguous(),
        stride=(stride, stride), padding=(1, 1))


def rows(y4):
    """[N,C,H,W] -> NHWC-flattened rows [N*H*W, C] (the kernels' y2d)."""
    return y4.permute(0, 2, 3, 1).reshape(-1, y4.shape[1])


def small_share(ref64):
    """Share of outputs with |ref| <= 256 (integers bf16 holds exactly)."""
    return (ref64.abs() <= 256).double().mean().item()


def check_budget(ref64, k, a, b, bf16_out):
    """Conditions on the REFERENCE, asserted before the kernel's output is
    looked at. k: reduction length; a, b: the operands. K*max|A|*max|B|
    bounds (|A| @ |B|^T).max() from above, so every partial sum in any
    order stays below 2^24; for a bf16 output at least 90% of the outputs
    are integers bf16 holds exactly, where a +-1 error cannot hide in the
    rounding."""
    assert torch.equal(ref64, ref64.round()), "reference is not integral"
    absprod = k * a.abs().max().item() * b.abs().max().item()
    assert absprod < TWO24, ("|A|.|B|^T budget", absprod)
    assert ref64.abs().max().item() < TWO24, "|ref| budget"
    if bf16_out:
        share = small_share(ref64)
        assert share >= 0.9, ("share of |ref| <= 256 below 90%", share)


def ref_stats(ref_rows64):
    """(sum y, sum y^2) per channel of the bf16-rounded reference rows
    [M, C], fp64; asserts that both (and sum |y|, which bounds every
    partial of sum y) stay below 2^24."""
    y = ref_rows64.to(torch.bfloat16).double()
    s, q = y.sum(0), (y * y).sum(0)
    assert y.abs().sum(0).max().item() < TWO24, "sum|y| budget"
    assert q.max().item() < TWO24, ("sum y^2 budget", q.max().item())
    return s, q


def check_exact(got, ref64, what=""):
    """fp32 got: bit-equal to ref64; bf16 got: bit-equal to ref64 rounded
    once (round-to-nearest-even) to bf16."""
    assert got.dtype in (torch.float32, torch.bfloat16), got.dtype
    assert tuple(got.shape) == tuple(ref64.shape), (got.shape, ref64.shape)
    want = ref64 if got.dtype == torch.float32 else ref64.to(torch.bfloat16)
    g = got.detach().cpu()
    if got.dtype == torch.float32:
        g = g.double()
    if torch.equal(g, want):
        return
    bad = (g != want).nonzero()
    first = [(tuple(i.tolist()), g[tuple(i)].item(), want[tuple(i)].item())
             for i in bad[:8]]
    raise AssertionError(
        f"{what}: {bad.shape[0]} of {g.numel()} elements differ from the "
        f"exact reference; the operands are exact integers, so the indices "
        f"point at the bug (tile, tail row, k-slice or tap). First "
        f"(index, got, want): {first}")


def accum_bound(absprod64, k):
    """E = 2*K*2^-24*(|A|.|B|^T): fp32 accumulation of K products in any
    order, factor 2 in case the MFMA accumulate truncates."""
    return 2.0 * k * 2.0 ** -24 * absprod64


def bound_ratio(got, ref64, absprod64, k):
    """max(err / bound) against the per-element bound: E for an fp32
    output, 2^-8*(|ref| + E) + E for a bf16 one."""
    e = accum_bound(absprod64, k)
    bound = e if got.dtype == torch.float32 else \
        2.0 ** -8 * (ref64.abs() + e) + e
    err = (got.detach().cpu().double() - ref64).abs()
    return (err / bound.clamp(min=1e-300)).max().item()
