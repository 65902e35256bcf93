"""bn_wide.hip: training BatchNorm(+ReLU) at C > 2048, one launch a pass,
against fp64 references computed on the CPU from the bf16 inputs.

Forward uses integer x in {-3..3}: per channel sum|x| and sum x^2 stay
below 2^24 (asserted on the reference), so both sums are exact in fp32 in
any order and the bounds of tests/test_bn_finalize_gpu.py carry over:
mean <= 2 ulp, invstd <= 2 ulp, running_var within that file's rv_bound,
y within its y_bound (6 * 2^-23 of the magnitude sum plus half a bf16 ulp).
rv_bound counts the roundings after an exact variance: the kernel forms
mean and the unbiased variance in double and rounds each to fp32 once.
running_mean = fma(mom, mean - rm, rm): 2 ulp of mean and 0.5 ulp of the
difference, scaled by mom, plus 0.5 ulp of the result. The ReLU mask must
equal (pre-activation > 0) wherever the reference pre-activation is
farther from 0 than y_bound, which at least 90% of the elements are.

Backward is real-valued. With u = 2^-24, a sum of M fp32 terms t_i in any
order, each carrying at most 3 roundings of its own (xhat = (x - mean) *
invstd is two, the product one), is within (M + 8) u sum|t_i|: M - 1
additions and 3 term roundings compound to (1 + u)^(M + 2) - 1 <= (M + 8) u
for M u < 0.01. That bounds dbeta (t = dy_eff) and dgamma (t = dy_eff *
xhat) by E1 and E2. dx = g * invstd * (dy_eff - s1/M - xhat * s2/M) is
within 2^-8 |dx| (the bf16 store) + g * invstd * (E1 + |xhat| E2) / M (the
sum errors carried through) + 8 u g invstd (|dy_eff| + |s1|/M + |xhat s2|/M)
(8 roundings in the bracket and the two scalings). mean and invstd are
given (fp64 from x, rounded to fp32) to kernel and reference alike. Each
test prints max(err / bound); docs/kernels.md ("bn_wide.hip") has them."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

MOM = float(torch.tensor(0.1, dtype=torch.float32).double())
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32).double())
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e():
    from edl_amd import ops
    return ops.ext()


def _ulp32(v64):
    """fp32 ulp of each |v| (fp64 tensor, normal range)."""
    _, e = torch.frexp(v64.abs().clamp(min=2.0 ** -120))
    return torch.ldexp(torch.ones_like(v64), e - 24)


def _rows(M, C, backward):
    """'cap' / 'cap+1': both sides of the resident / streaming switch."""
    if isinstance(M, int):
        return M
    cap = _e().bn_wide_resident_rows(C, backward)
    assert 0 < cap <= 4096, cap  # {-3..3} keeps sum x^2 < 2^24 up to there
    return cap + (M == "cap+1")


def _ref_fwd(x, gamma, beta, rm0, rv0, relu):
    """fp64 forward of x (bf16 [M, C], integer-valued) with its bounds."""
    xd, g, b = x.double(), gamma.double(), beta.double()
    M = xd.shape[0]
    assert xd.abs().sum(0).max().item() < 2 ** 24, "sum|x| budget"
    assert (xd * xd).sum(0).max().item() < 2 ** 24, "sum x^2 budget"
    mean = xd.sum(0) / M
    var = (xd * xd).sum(0) / M - mean * mean
    assert var.min().item() > 0, "degenerate case: var <= 0"
    invstd = (var + EPS32).rsqrt()
    rm = rm0.double() + MOM * (mean - rm0.double())
    rm_bound = (MOM * (2 * _ulp32(mean) + 0.5 * _ulp32(mean - rm0.double()))
                + 0.5 * _ulp32(rm))
    ub = var * M / (M - 1)
    rv = rv0.double() + MOM * (ub - rv0.double())
    rv_bound = (MOM * (0.5 * _ulp32(ub) + 0.5 * _ulp32(ub - rv0.double()))
                + 0.5 * _ulp32(rv))
    scale = g * invstd
    pre = xd * scale + (b - scale * mean)
    y = pre.clamp(min=0) if relu else pre
    y_bound = 2.0 ** -8 * y.abs() + 6 * 2.0 ** -23 * (
        xd.abs() * scale + b.abs() + scale * mean.abs())
    sure = pre.abs() > y_bound
    assert sure.double().mean().item() >= 0.9, "mask check covers too little"
    return dict(mean=mean, invstd=invstd, rm=rm, rm_bound=rm_bound, rv=rv,
                rv_bound=rv_bound, y=y, y_bound=y_bound, pos=pre > 0,
                sure=sure)


def _ref_bwd(dy, bits, x, mean, invstd, gamma):
    """fp64 backward and its bounds; bits: bool [M, C] ReLU mask or None."""
    g = dy.double() if bits is None else dy.double() * bits.double()
    M = g.shape[0]
    xhat = (x.double() - mean.double()) * invstd.double()
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    e1 = (M + 8) * U * g.abs().sum(0)
    e2 = (M + 8) * U * (g * xhat).abs().sum(0)
    k = gamma.double() * invstd.double()
    dx = k * (g - s1 / M - xhat * s2 / M)
    dx_bound = (2.0 ** -8 * dx.abs() + k * (e1 + xhat.abs() * e2) / M
                + 8 * U * k * (g.abs() + s1.abs() / M + (xhat * s2).abs() / M))
    return dict(dbeta=s1, dbeta_bound=e1, dgamma=s2, dgamma_bound=e2, dx=dx,
                dx_bound=dx_bound)


def _ratios(tag, ref, **got):
    """Print and assert max(err / bound) of every named quantity (0 where
    the result is exact: a fully masked channel has bound 0)."""
    out = {}
    for n, t in got.items():
        err = (t.detach().cpu().double() - ref[n]).abs()
        out[n] = torch.where(err > 0, err / ref[n + "_bound"],
                             torch.zeros_like(err)).max().item()
    print(tag, " ".join(f"{n} {v:.3f}" for n, v in out.items()))
    assert max(out.values()) <= 1.0, out


W8 = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128])  # bit k = channel 8o + k


def _pack(bits):  # bool [M, C] -> the kernels' mask bytes [M, C/8]
    return (bits.view(len(bits), -1, 8).long() * W8).sum(-1).to(torch.uint8)


def _unpack(mask):
    return ((mask.cpu().long().unsqueeze(-1) & W8) != 0).flatten(1)


@functools.lru_cache(maxsize=None)
def _inputs(M, C):
    gen = torch.Generator().manual_seed(4000 + 7 * M + C)
    f = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    n = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    xi = torch.randint(-3, 4, (M, C), generator=gen)
    flat = (xi == xi[0]).all(0)  # M = 2: a constant channel has var = 0
    xi[0, flat] = (xi[0, flat] + 4) % 7 - 3  # the next value of {-3..3}
    return dict(
        xi=xi.to(torch.bfloat16),
        x=n(M, C).to(torch.bfloat16), dy=n(M, C).to(torch.bfloat16),
        bits=torch.rand(M, C, generator=gen) < 0.5,
        gamma=f(C) + 0.5, beta=n(C), rm0=n(C), rv0=f(C) + 0.5)


CASES = [(2, 2112, True), (49, 4096, True), (49, 4096, False),
         (197, 2112, True), ("cap", 2112, True), ("cap+1", 2112, True)]


@pytest.mark.parametrize("M,C,relu", CASES)
def test_forward_integer_exact(M, C, relu):
    M = _rows(M, C, 0)
    k = _inputs(M, C)
    ref = _ref_fwd(k["xi"], k["gamma"], k["beta"], k["rm0"], k["rv0"], relu)
    rm, rv = k["rm0"].cuda(), k["rv0"].cuda()
    y, mean, invstd, mask = _e().bn_wide_fwd_train(
        k["xi"].cuda(), k["gamma"].cuda(), k["beta"].cuda(), rm, rv, MOM,
        1e-5, relu)
    ref["mean_bound"] = 2 * _ulp32(ref["mean"])
    ref["invstd_bound"] = 2 * _ulp32(ref["invstd"])
    _ratios(f"fwd M={M} C={C} relu={relu}:", ref, mean=mean, invstd=invstd,
            rm=rm, rv=rv, y=y)
    if relu:
        assert tuple(mask.shape) == (M, C // 8) and mask.dtype == torch.uint8
        wrong = (_unpack(mask) != ref["pos"]) & ref["sure"]
        assert not wrong.any(), f"{int(wrong.sum())} mask bits differ"
    else:
        assert mask.numel() == 0


@pytest.mark.parametrize("M,C,relu,acc", [c + (False,) for c in CASES] +
                         [(197, 2112, True, True)])
def test_backward(M, C, relu, acc):
    M = _rows(M, C, 1)
    k = _inputs(M, C)
    xd = k["x"].double()
    mean = xd.mean(0).float()
    invstd = (xd.var(0, unbiased=False) + EPS32).rsqrt().float()
    bits = k["bits"] if relu else None
    ref = _ref_bwd(k["dy"], bits, k["x"], mean, invstd, k["gamma"])
    args = [k["dy"].cuda(), _pack(bits).cuda() if relu else None,
            k["x"].cuda(), mean.cuda(), invstd.cuda(), k["gamma"].cuda(), relu]
    if acc:  # direct-grad accumulators preloaded with small integers
        ch = torch.arange(C)
        pre_g, pre_b = (ch % 11 - 5).float(), (ch % 13 - 6).float()
        gacc, bacc = pre_g.cuda(), pre_b.cuda()
        args += [gacc, bacc]
    dx, dgamma, dbeta = _e().bn_wide_bwd(*args)
    _ratios(f"bwd M={M} C={C} relu={relu} acc={acc}:", ref, dx=dx,
            dgamma=dgamma, dbeta=dbeta)
    if acc:  # acc = fl(pre + sum): the sum's bound plus the add's rounding
        for name, a, pre in (("dgamma", gacc, pre_g), ("dbeta", bacc, pre_b)):
            want = pre.double() + ref[name]
            err = (a.cpu().double() - want).abs()
            assert (err <= ref[name + "_bound"] + 0.5 * _ulp32(want)).all(), name


def test_forced_w64(monkeypatch):  # the slab width the launcher leaves out
    monkeypatch.setenv("EDL_BN_WIDE_W", "64")
    test_forward_integer_exact(197, 2112, True)
    test_backward(197, 2112, True, False)
    test_backward("cap", 2112, True, False)


@pytest.mark.parametrize("cls,switch,calls", [
    ("BNReLU2d", "1", 1), ("BNReLU2d", "0", 0), ("BNAddReLU2d", "1", 0),
    ("BNAddReLU2d", "0", 0)])
def test_module_route(monkeypatch, cls, switch, calls):
    from edl_amd.ops import bnrelu
    C, e, seen = 4096, _e(), {"bn_wide_fwd_train": [], "bn_wide_bwd": []}

    def counted(name, fn):
        def f(*a):
            seen[name].append(fn(*a))
            return seen[name][-1]
        return f

    for name in seen:
        monkeypatch.setattr(e, name, counted(name, getattr(e, name)))
    monkeypatch.setenv("EDL_BN_WIDE_TRAIN", switch)
    k = _inputs(98, C)
    cl = lambda t: (t.view(2, 7, 7, C).permute(0, 3, 1, 2).cuda()  # noqa: E731
                    .contiguous(memory_format=torch.channels_last))
    m = getattr(bnrelu, cls)(C).cuda().train()
    with torch.no_grad():
        m.weight.copy_(k["gamma"])
        m.bias.copy_(k["beta"])
        m.running_mean.copy_(k["rm0"])
        m.running_var.copy_(k["rv0"])
    x = cl(k["xi"]).requires_grad_(True)
    y = m(x) if cls == "BNReLU2d" else m(x, cl(k["x"]))
    y.backward(cl(k["dy"]))
    assert [len(v) for v in seen.values()] == [calls, calls], seen.keys()
    assert m._batches_seen == 1 and x.grad is not None
    if not calls:
        return
    fref = _ref_fwd(k["xi"], k["gamma"], k["beta"], k["rm0"], k["rv0"], True)
    to2d = lambda t: t.permute(0, 2, 3, 1).reshape(98, C)  # noqa: E731
    _ratios("module fwd:", fref, y=to2d(y), rm=m.running_mean,
            rv=m.running_var)
    # backward against the statistics and the mask the forward handed on
    _, mean, invstd, mask = seen["bn_wide_fwd_train"][0]
    ref = _ref_bwd(k["dy"], _unpack(mask), k["xi"], mean.cpu(), invstd.cpu(),
                   k["gamma"])
    _ratios("module bwd:", ref, dx=to2d(x.grad), dgamma=m.weight.grad,
            dbeta=m.bias.grad)


SPOIL = {  # what each refusal case does to the operands
    "dtype": lambda a: a.update(x=a["x"].float()),
    "device": lambda a: a.update(x=a["x"].cpu()),
    "layout": lambda a: a.update(
        x=torch.empty_like(a["x"].t().contiguous()).t()),
    "mask": lambda a: a.update(mask=a["mask"][1:]),
    None: lambda a: None}


@pytest.mark.parametrize("M,C,spoil,match", [
    (4, 4096, "dtype", "bf16"), (4, 4096, "device", "GPU"),
    (4, 4096, "layout", "contiguous"), (4, 2048, None, "C > 2048"),
    (4, 4128, None, "C % 64"), (1, 4096, None, "2 <= M"),
    (4, 4096, "mask", "mask")])
def test_refusals(M, C, spoil, match):
    a = dict(x=torch.zeros(M, C, device="cuda", dtype=torch.bfloat16),
             mask=torch.zeros(M, C // 8, device="cuda", dtype=torch.uint8))
    dy = a["x"].clone()
    SPOIL[spoil](a)
    one = torch.ones(C, device="cuda")
    if spoil != "mask":
        with pytest.raises(RuntimeError, match=match):
            _e().bn_wide_fwd_train(a["x"], one, one, one.clone(), one.clone(),
                                   0.1, 1e-5, True)
    with pytest.raises(RuntimeError, match=match):
        _e().bn_wide_bwd(dy, a["mask"], a["x"], one, one, one, True)


def test_graph_replay():
    """Forward + backward of the (49, 4096) calls captured on one stream:
    two replays with new contents in the static inputs, each bit-equal to
    the eager calls (nothing in the kernels is atomic)."""
    M, C = 49, 4096
    k, e = _inputs(M, C), _e()
    x, dy = k["xi"].cuda(), k["dy"].cuda()
    gamma, beta = k["gamma"].cuda(), k["beta"].cuda()
    rm, rv = k["rm0"].cuda(), k["rv0"].cuda()

    def run():
        y, mean, invstd, mask = e.bn_wide_fwd_train(x, gamma, beta, rm, rv,
                                                    MOM, 1e-5, True)
        return (y, mean, invstd, mask) + tuple(
            e.bn_wide_bwd(dy, mask, x, mean, invstd, gamma, True))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # loads the code outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for it in range(2):
        x.copy_(_inputs(M + 1 + it, C)["xi"][:M])
        dy.copy_(_inputs(M + 1 + it, C)["dy"][:M])
        rm.copy_(k["rm0"]), rv.copy_(k["rv0"])
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs] + [rm.clone(), rv.clone()]
        rm.copy_(k["rm0"]), rv.copy_(k["rv0"])
        want = list(run()) + [rm, rv]
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), f"replay {it}: output {i} differs"
