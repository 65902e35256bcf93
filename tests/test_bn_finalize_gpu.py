"""The two BN finalize kernels (bnrelu.hip: bn_finalize_kernel,
bn_bwd_finalize_kernel) on integer partials, where every sum is exact in
fp32 in ANY order: a dropped, doubled or misplaced partial row moves the
result instead of hiding in a tolerance (idiom of _mfma_exact_common.py).

The forward kernel reduces [rows, 2C] partials with 1024-thread blocks
(64 channels x 16 row strips, one batch of loads up to 192 rows, 4-row
and 1-row batches for the short partials), the backward one with 64
columns x 4 strips, 8 rows a round; the row counts below sit on both
sides of every batch and strip boundary.

Bounds that are not bit-equality are derived from operation counts:
  invstd = rsqrtf(var + eps): the add rounds once (relative 2^-24, halved
    by the inverse square root: <= 0.5 ulp of the result) and rsqrtf is
    a 1-ulp function (HIP math API) -> 1.5 ulp, asserted as 2.
  mean at M != 2^k: inv_m = 1/M rounds once, s * inv_m once -> 2 ulp.
  running_var = fma(mom, ub - rv, rv), ub = var * M / (M - 1): the
    division and the subtraction round once each (0.5 ulp of ub and of
    ub - rv, scaled by mom), the fma once (0.5 ulp of the result).
  y = bf16(fma(x, scale, shift)), scale = g * invstd (2 ulp), shift =
    beta - scale * mean (2.5 ulp of the product, 0.5 of the difference),
    fma 0.5: <= 6 * 2^-23 * (|x| |scale| + |beta| + |scale| |mean|),
    plus half a bf16 ulp of the result, 2^-8 |y|.
Each test prints its measured maximum before asserting; docs/kernels.md
("bnrelu.hip") records them.
"""
import functools

import pytest
import torch

import _mfma_exact_common as X

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e():
    from edl_amd import ops
    return ops.ext()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ulp32(v64):
    """fp32 ulp of each |v| (fp64 tensor, normal range)."""
    _, e = torch.frexp(v64.abs().clamp(min=2.0 ** -120))
    return torch.ldexp(torch.ones_like(v64), e - 24)


def _is_f32(v64):
    return torch.equal(v64.float().double(), v64)


M_FWD = 16
MOM = 0.5
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32).double())

ROWS = [1, 3, 4, 15, 16, 17, 63, 64, 65, 191, 192, 193, 512]
CHANS = [8, 64, 128, 2048]


@functools.lru_cache(maxsize=None)
def _fwd_case(rows, C):
    """Operands and fp64 references of one forward finalize; budgets are
    asserted on the reference before any kernel output is looked at."""
    gen = _gen(7000 + 31 * rows + C)
    s = torch.tensor(X.PM12, dtype=torch.float64)[
        torch.randint(4, (rows, C), generator=gen)]
    q = s * s + torch.randint(4, (rows, C), generator=gen).double()
    P = torch.cat([s, q], 1).float()
    x = X.ints((M_FWD, C), X.ASYM3, gen)
    ch = torch.arange(C)
    gamma = (1 + ch % 4).float()
    beta = (ch % 5 - 2).float()
    rm0 = (ch % 7 - 3).float()
    rv0 = torch.ones(C)

    S, Q = s.sum(0), q.sum(0)
    # |sum s| < 2^12: mean = k/16 and mean^2 = k^2/256 are exact, and with
    # 16 sum q < 2^24 so are q/16 and var = (16 q - k^2)/256
    assert s.abs().sum(0).max().item() < 4096, "sum|s| budget"
    assert 16 * Q.max().item() < X.TWO24, "sum q budget"
    mean = S / M_FWD
    var = Q / M_FWD - mean * mean
    assert _is_f32(mean) and _is_f32(var) and _is_f32(mean * mean)
    assert var.min().item() > 0, "degenerate case: var <= 0"
    invstd = (var + EPS32).rsqrt()
    rm = rm0.double() + MOM * (mean - rm0.double())
    assert _is_f32(rm), "running_mean reference not exact"
    ub = var * M_FWD / (M_FWD - 1)
    rv = rv0.double() + MOM * (ub - rv0.double())
    rv_bound = (MOM * (0.5 * _ulp32(ub) + 0.5 * _ulp32(ub - rv0.double()))
                + 0.5 * _ulp32(rv))
    scale = gamma.double() * invstd
    xd = x.double()
    y = xd * scale + (beta.double() - scale * mean)
    y_bound = (2.0 ** -8 * y.abs() + 6 * 2.0 ** -23 * (
        xd.abs() * scale + beta.double().abs() + scale * mean.abs()))
    return dict(P=P, x=x, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0,
                mean=mean, invstd=invstd, rm=rm, rv=rv, rv_bound=rv_bound,
                y=y, y_bound=y_bound)


@pytest.mark.parametrize("C", CHANS)
@pytest.mark.parametrize("rows", ROWS)
def test_fwd_finalize_exact(rows, C):
    k = _fwd_case(rows, C)
    P = k["P"].cuda()
    rm, rv = k["rm0"].cuda(), k["rv0"].cuda()
    y, mean, invstd, _ = _e().bn_fwd_train(
        k["x"].cuda(), k["gamma"].cuda(), k["beta"].cuda(), rm, rv, MOM,
        1e-5, None, False, P)
    X.check_exact(mean, k["mean"], f"mean rows={rows} C={C}")
    X.check_exact(rm, k["rm"], f"running_mean rows={rows} C={C}")
    inv_ulps = ((invstd.cpu().double() - k["invstd"]).abs() /
                _ulp32(k["invstd"])).max().item()
    rv_ratio = ((rv.cpu().double() - k["rv"]).abs() /
                k["rv_bound"]).max().item()
    y_ratio = ((y.cpu().double() - k["y"]).abs() / k["y_bound"]).max().item()
    print(f"fwd rows={rows} C={C}: invstd {inv_ulps:.3f} ulp, running_var "
          f"{rv_ratio:.3f} of bound, y {y_ratio:.3f} of bound")
    assert inv_ulps <= 2.0, inv_ulps
    assert rv_ratio <= 1.0, rv_ratio
    assert y_ratio <= 1.0, y_ratio
    # a hand-made partial is not pooled: read only
    assert torch.equal(P.cpu(), k["P"]), "non-pooled pre_part was modified"


# ---- zero-after-read of the pooled (capped, atomically folded) partials ----

@functools.lru_cache(maxsize=None)
def _stats_case(M):
    """gemm_bt_stats operands (N = K = 64: 256-row tiles) and the exact
    (sum y, sum y^2) of its output."""
    gen = _gen(9000 + M)
    a = X.ints((M, 64), X.PM1, gen)
    b = X.ints((64, 64), X.PM1, gen)
    ref = X.exact_ref_bt(a, b)
    s, q = X.ref_stats(ref)  # asserts the 2^24 budget of both sums
    return a.cuda(), b.cuda(), s, q


def _bn_consume(c, part):
    C = c.shape[1]
    f = dict(device="cuda", dtype=torch.float32)
    _, mean, invstd, _ = _e().bn_fwd_train(
        c, torch.ones(C, **f), torch.zeros(C, **f), torch.zeros(C, **f),
        torch.ones(C, **f), 0.1, 1e-5, None, True, part)
    return mean, invstd


def test_pooled_partial_zeroed_after_read():
    """M = 50000 rows are 196 tiles of 256 > the 192-row cap, so the
    partials are the pooled buffer (M = 25000 would be 98 tiles: that is
    the non-pooled case below)."""
    M = 50000
    a, b, s, q = _stats_case(M)
    assert -(-M // 256) > 192
    got = []
    part = None
    try:
        for it in range(2):
            c, part = _e().gemm_bt_stats(a, b)
            assert tuple(part.shape) == (192, 128)
            folded = part.double().sum(0).cpu()
            assert torch.equal(folded[:64], s) and torch.equal(folded[64:], q)
            mean, invstd = _bn_consume(c, part)
            assert not part.any(), f"round {it}: pooled partial left dirty"
            got.append((mean.cpu(), invstd.cpu()))
    finally:
        if part is not None:
            part.zero_()  # a failure must not poison the shared pool
    assert torch.equal(got[0][0], got[1][0]), "mean differs in round 2"
    assert torch.equal(got[0][1], got[1][1]), "invstd differs in round 2"
    mean64 = s / M
    mean_ulps = ((got[0][0].double() - mean64).abs() /
                 _ulp32(mean64)).max().item()
    print(f"pooled M={M}: mean {mean_ulps:.3f} ulp")
    assert mean_ulps <= 2.0, mean_ulps


def test_unpooled_partial_unmodified():
    M = 25000
    a, b, s, q = _stats_case(M)
    c, part = _e().gemm_bt_stats(a, b)
    assert tuple(part.shape) == (98, 128)
    before = part.clone()
    mean, _ = _bn_consume(c, part)
    assert torch.equal(part, before), "non-pooled pre_part was modified"
    mean64 = s / M
    assert ((mean.cpu().double() - mean64).abs() /
            _ulp32(mean64)).max().item() <= 2.0


# ---- backward ----

def _bwd_rows(M, C):
    """bn_bwd_grid (bnrelu.hip) at the default cap."""
    rpb = max(256 // (C // 8), 1)
    cap = max(min(131072 // (2 * C), 192), 8)
    return max(min(-(-M // rpb), cap), 1)


# (M, C, partial rows)
BWD_CASES = [(32, 64, 1), (150, 64, 5), (1056, 64, 33), (6144, 64, 192),
             (600, 512, 128), (40, 2048, 32)]


@functools.lru_cache(maxsize=None)
def _bwd_case(M, C):
    gen = _gen(8000 + M + C)
    dy = X.ints((M, C), X.PM1, gen)
    x = X.ints((M, C), X.ASYM3, gen)
    mean = (torch.arange(C) % 3 - 1).float()
    xhat = x.double() - mean.double()
    assert M * xhat.abs().max().item() < X.TWO24, "sum budget"
    s1 = dy.double().sum(0)
    s2 = (dy.double() * xhat).sum(0)
    return dy.cuda(), x.cuda(), mean.cuda(), s1, s2


@pytest.mark.parametrize("M,C,rows", BWD_CASES)
def test_bwd_finalize_exact(M, C, rows):
    assert _bwd_rows(M, C) == rows
    dy, x, mean, s1, s2 = _bwd_case(M, C)
    f = dict(device="cuda", dtype=torch.float32)
    one = torch.ones(C, **f)
    _, dgamma, dbeta, _ = _e().bn_bwd(dy, None, x, mean, one, one, False,
                                      False, True)
    X.check_exact(dbeta, s1, f"dbeta M={M} C={C}")
    X.check_exact(dgamma, s2, f"dgamma M={M} C={C}")

    # direct-grad accumulators: preset + sum, nothing outside [C] touched
    G = 8
    ch = torch.arange(C)
    pre_g, pre_b = (ch % 11 - 5).double(), (ch % 13 - 6).double()
    assert (pre_g.abs() + s2.abs()).max().item() < X.TWO24
    assert (pre_b.abs() + s1.abs()).max().item() < X.TWO24
    gbuf = torch.full((C + 2 * G,), 7.0, **f)
    bbuf = torch.full((C + 2 * G,), -9.0, **f)
    gacc, bacc = gbuf[G:G + C], bbuf[G:G + C]
    gacc.copy_(pre_g.float())
    bacc.copy_(pre_b.float())
    _e().bn_bwd(dy, None, x, mean, one, one, False, False, True, gacc, bacc)
    X.check_exact(gacc, pre_g + s2, f"dgamma_acc M={M} C={C}")
    X.check_exact(bacc, pre_b + s1, f"dbeta_acc M={M} C={C}")
    for buf, v in ((gbuf, 7.0), (bbuf, -9.0)):
        assert (buf[:G] == v).all() and (buf[G + C:] == v).all(), \
            "accumulator guard elements were written"


# ---- graph replay ----

def _capture(run):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # allocates the pool and loads the code outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    return g, outs


def test_finalize_graph_replay():
    """One pooled forward finalize (re-armed by its producer inside the
    graph) and one backward finalize: three replays, each bit-equal to the
    eager call."""
    a, b, _, _ = _stats_case(50000)
    dy, x, mean_b, _, _ = _bwd_case(6144, 64)
    one = torch.ones(64, device="cuda")

    def run():
        c, part = _e().gemm_bt_stats(a, b)
        mean, invstd = _bn_consume(c, part)
        dx, dgamma, dbeta, _ = _e().bn_bwd(dy, None, x, mean_b, one, one,
                                           False, False, True)
        return mean, invstd, dx, dgamma, dbeta

    part = _e().gemm_bt_stats(a, b)[1]
    try:
        _bn_consume(_e().gemm_bt(a, b), part)  # leave the pool clean
        eager = [t.clone() for t in run()]
        g, outs = _capture(run)
        for it in range(3):
            g.replay()
            torch.cuda.synchronize()
            for name, e, o in zip(("mean", "invstd", "dx", "dgamma", "dbeta"),
                                  eager, outs):
                assert torch.equal(e, o), f"replay {it}: {name} differs"
            assert not part.any(), f"replay {it}: pooled partial left dirty"
    finally:
        part.zero_()
