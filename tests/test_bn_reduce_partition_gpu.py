"""The channel-slab x row partition of bn_stats and bn_bwd_reduce
(bnrelu.hip: bn_stats_slab_kernel, bn_bwd_reduce_slab_kernel, planned by
bn_reduce_plan) on integer operands, where every per-channel sum is exact
in fp32 in ANY order (idiom of _mfma_exact_common.py): a row visited twice,
a row missed, a masked tail row that still adds, or a slab stored into the
wrong columns of the partial moves the result instead of hiding in a
tolerance.

The plan is mirrored in _plan below and the mirror held to a table; the M
values of every C are derived from it: one row, the rows of one block pass
-1 / +0 / +1, one full 4-row round at R = 1 (with several slabs from
C = 128 up), the M at which R first reaches its cap and one pass beyond,
an M that runs the unmasked main loop and the masked tail round, and both
sides of every M at which the plan changes the block size.

What is not bit-equality is the real-valued case: fp32 accumulation of M
terms in any order is within M * 2^-24 * sum|term| per channel of the fp64
sum of the same terms. The test prints the measured max(err / bound) before
asserting; docs/kernels.md ("bnrelu.hip") records it.
"""
import functools

import pytest
import torch

import _mfma_exact_common as X

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    # the slab partition is what this file tests, whatever the caller's
    # environment says (the row-only fold uses LDS atomics: exact on
    # integers, not bit-stable between two calls on real values)
    monkeypatch.setenv("EDL_BN_SLAB", "1")


def _e():
    from edl_amd import ops
    return ops.ext()


R_CAP = 192        # partial rows: one load batch of the forward finalize
SLAB_BLOCKS = 1024  # R * S bound
SLAB_WAVES = 4096   # bound on the grid when the block grows


def _plan(M, C):
    """bn_reduce_plan (bnrelu.hip) at the default caps ->
    (R, S, Cs, threads per block)."""
    Cs = min(C, 64)
    S = C // Cs
    c8s = Cs // 8
    rcap = max(min(SLAB_BLOCKS // S, R_CAP), 1)
    nthr = 256
    while True:
        rpb = nthr // c8s
        R = min(max(-(-M // (4 * rpb)), 1), rcap)
        if (nthr == 1024 or M <= 8 * R * rpb
                or R * S * (2 * nthr // 64) > SLAB_WAVES):
            return R, S, Cs, nthr
        nthr *= 2


# (M, C) -> (R, S, Cs, threads): the ResNet50_vd batch-32 layer classes and
# the corners of the plan, worked out by hand from the rules in bnrelu.hip
PLAN_TABLE = {
    (1, 8): (1, 1, 8, 256),
    (1568, 2048): (13, 32, 64, 256),
    (1568, 512): (13, 8, 64, 256),
    (6272, 1024): (49, 16, 64, 256),
    (6272, 256): (49, 4, 64, 256),
    (25088, 512): (128, 8, 64, 256),
    (25088, 128): (192, 2, 64, 256),
    (100352, 256): (192, 4, 64, 256),
    (100352, 128): (192, 2, 64, 512),
    (100352, 64): (192, 1, 64, 1024),
    (401408, 64): (192, 1, 64, 1024),
    (401408, 32): (192, 1, 32, 1024),
    (3968, 2048): (31, 32, 64, 256),
    (3969, 2048): (32, 32, 64, 256),
    (49152, 128): (192, 2, 64, 256),
    (49153, 128): (192, 2, 64, 512),
    (98304, 64): (192, 1, 64, 512),
    (98305, 64): (192, 1, 64, 1024),
}


def test_plan_mirror_matches_table():
    for (M, C), want in PLAN_TABLE.items():
        assert _plan(M, C) == want, (M, C, _plan(M, C), want)


CHANS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048]


def _m_values(C):
    Cs = min(C, 64)
    S = C // Cs
    rpb = 256 // (Cs // 8)            # rows of one block pass, 256 threads
    rcap = max(min(SLAB_BLOCKS // S, R_CAP), 1)
    m_cap = (rcap - 1) * 4 * rpb + 1  # R first reaches its cap
    ms = [1, rpb - 1, rpb, rpb + 1,
          4 * rpb,                    # one full round, R = 1 (S > 1: C >= 128)
          m_cap, m_cap + rpb,
          4 * rcap * rpb + rpb + 3]   # unmasked main loop + masked tail
    assert _plan(4 * rpb, C)[:2] == (1, S)
    assert _plan(m_cap - 1, C)[0] == rcap - 1 and _plan(m_cap, C)[0] == rcap
    nthr = 256
    while nthr < 1024 and rcap * S * (2 * nthr // 64) <= SLAB_WAVES:
        m_thr = 8 * rcap * (nthr // (Cs // 8))  # last M at this block size
        assert _plan(m_thr, C)[3] == nthr and _plan(m_thr + 1, C)[3] == 2 * nthr
        ms += [m_thr, m_thr + 1]
        nthr *= 2
    return sorted(set(m for m in ms if m >= 1))


CASES = [(M, C) for C in CHANS for M in _m_values(C)]


def test_cases_cover_every_path():
    blocks = {_plan(M, C)[3] for M, C in CASES}
    slabs = {_plan(M, C)[1] for M, C in CASES}
    assert blocks == {256, 512, 1024} and slabs == {1, 2, 4, 8, 16, 32}
    # the largest case stays small: about 10 M elements
    assert max(M * C for M, C in CASES) <= 11 << 20


def _ints(shape, values, gen):
    """X.ints on the GPU: bf16 drawn uniformly from a set of non-zero
    integers."""
    table = torch.tensor(values, dtype=torch.float32, device="cuda")
    idx = torch.randint(len(values), tuple(shape), generator=gen,
                        device="cuda")
    return table[idx].to(torch.bfloat16)


def _bits(mask, M, C):
    """[M, C/8] mask bytes -> [M, C] 0/1 (bit k of byte [row, oct] is
    channel oct * 8 + k)."""
    b = (mask.view(M, C // 8, 1).int() >>
         torch.arange(8, device="cuda", dtype=torch.int32)) & 1
    return b.view(M, C)


@functools.lru_cache(maxsize=None)  # about 1 GB of operands over all CASES
def _case(M, C):
    """Operands of one (M, C) and the fp64 references of the backward sums,
    with and without the ReLU mask; the 2^24 budgets are asserted on the
    references before any kernel output is looked at."""
    gen = torch.Generator(device="cuda").manual_seed(6000 + 7 * M + C)
    dy = _ints((M, C), X.PM1, gen)
    x = _ints((M, C), X.ASYM3, gen)
    mask = torch.randint(256, (M, C // 8), generator=gen, device="cuda",
                         dtype=torch.uint8)
    mean = (torch.arange(C, device="cuda") % 3 - 1).float()
    xhat = x.double() - mean.double()
    assert M * xhat.abs().max().item() < X.TWO24, "sum budget"
    refs = {}
    for relu in (False, True):
        g = dy.double()
        if relu:
            g = g * _bits(mask, M, C)
        refs[relu] = (g.sum(0).cpu(), (g * xhat).sum(0).cpu())
    return dict(dy=dy, x=x, mask=mask, mean=mean, refs=refs)


VARIANTS = [(True, False), (True, True), (False, False)]  # (relu, add)


@pytest.mark.parametrize("M,C", CASES)
def test_backward_sums_exact_and_old_equals_new(M, C, monkeypatch):
    k = _case(M, C)
    one = torch.ones(C, device="cuda")
    for relu, add in VARIANTS:
        s1, s2 = k["refs"][relu]
        got = {}
        for slab in ("1", "0"):
            monkeypatch.setenv("EDL_BN_SLAB", slab)
            got[slab] = _e().bn_bwd(k["dy"], k["mask"] if relu else None,
                                    k["x"], k["mean"], one, one, relu, add,
                                    True, None, None)
        what = f"M={M} C={C} relu={relu} add={add}"
        dx, dgamma, dbeta, dres = got["1"]
        X.check_exact(dbeta, s1, "dbeta " + what)
        X.check_exact(dgamma, s2, "dgamma " + what)
        names = ("dx", "dgamma", "dbeta") + (("dres",) if add else ())
        for name, a, b in zip(names, got["1"], got["0"]):
            assert torch.equal(a, b), f"{name} differs old/new: {what}"


@pytest.mark.parametrize("M,C", CASES)
def test_forward_stats_exact(M, C):
    k = _case(M, C)
    x = k["x"]
    xd = x.double()
    assert 9 * M < X.TWO24, "sum x^2 budget"
    s = xd.sum(0).float()  # exact integers
    f = dict(device="cuda", dtype=torch.float32)
    _, mean, invstd, _ = _e().bn_fwd_train(
        x, torch.ones(C, **f), torch.zeros(C, **f), torch.zeros(C, **f),
        torch.ones(C, **f), 0.1, 1e-5, None, True, None)
    # the kernel's expression, in fp32: mean = sum * (1 / M)
    inv_m = (torch.tensor(1.0, dtype=torch.float32) / M).cuda()
    assert torch.equal(mean, s * inv_m), (mean - s * inv_m).abs().max().item()
    ref = torch.rsqrt(xd.var(0, unbiased=False) + 1e-5)
    if M > 1:  # sum x^2 too: invstd within the finalize's rounding of it
        assert torch.allclose(invstd.double(), ref, rtol=1e-5, atol=0), \
            (invstd.double() / ref - 1).abs().max().item()


# one case per block size and per slab count that ships
REAL_CASES = [(500, 32), (98305, 64), (49153, 128), (300, 256), (300, 512),
              (300, 1024), (300, 2048)]


@pytest.mark.parametrize("M,C", REAL_CASES)
def test_real_values_within_accumulation_bound(M, C):
    gen = torch.Generator(device="cuda").manual_seed(77 + M + C)

    def rn(*shape):
        return torch.randn(*shape, generator=gen, device="cuda")

    dy, x = rn(M, C).to(torch.bfloat16), rn(M, C).to(torch.bfloat16)
    mask = torch.randint(256, (M, C // 8), generator=gen, device="cuda",
                         dtype=torch.uint8)
    mean = rn(C) * 0.1
    invstd = torch.rand(C, generator=gen, device="cuda") + 0.5
    one = torch.ones(C, device="cuda")
    g = dy.double() * _bits(mask, M, C)
    t2 = g * ((x.double() - mean.double()) * invstd.double())
    a = _e().bn_bwd(dy, mask, x, mean, invstd, one, True, False, True, None,
                    None)
    b = _e().bn_bwd(dy, mask, x, mean, invstd, one, True, False, True, None,
                    None)
    ratio = 0.0
    for got, terms in ((a[2], g), (a[1], t2)):
        bound = M * 2.0 ** -24 * terms.abs().sum(0)
        err = (got.double() - terms.sum(0)).abs()
        ratio = max(ratio, (err / bound.clamp(min=1e-300)).max().item())
    print(f"real M={M} C={C} plan={_plan(M, C)}: max err/bound {ratio:.4f}")
    assert ratio <= 1.0, ratio
    for name, u, v in zip(("dx", "dgamma", "dbeta"), a, b):
        assert torch.equal(u, v), f"{name}: two calls differ"


def _capture(run):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # loads the code outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    return g, outs


def test_graph_replay():
    """One slab-split backward (C = 1024: 16 slabs) and one narrow one:
    three replays, each bit-equal to the eager call."""
    wide, narrow = _case(129, 1024), _case(6145, 64)
    assert _plan(129, 1024)[:2] == (2, 16) and _plan(6145, 64)[:2] == (49, 1)

    def run():
        outs = []
        for k, C in ((wide, 1024), (narrow, 64)):
            one = torch.ones(C, device="cuda")
            dx, dgamma, dbeta, _ = _e().bn_bwd(
                k["dy"], k["mask"], k["x"], k["mean"], one, one, True, False,
                True, None, None)
            outs += [dx, dgamma, dbeta]
        return outs

    eager = [t.clone() for t in run()]
    g, outs = _capture(run)
    for it in range(3):
        g.replay()
        torch.cuda.synchronize()
        for i, (e, o) in enumerate(zip(eager, outs)):
            assert torch.equal(e, o), f"replay {it}: output {i} differs"


def test_accumulator_guard_elements():
    """Direct-grad accumulators of a slab-split shape: preset + sum, and
    nothing outside [C] written."""
    M, C, G = 129, 1024, 8
    k = _case(M, C)
    s1, s2 = k["refs"][False]
    f = dict(device="cuda", dtype=torch.float32)
    one = torch.ones(C, **f)
    ch = torch.arange(C)
    pre_g, pre_b = (ch % 11 - 5).double(), (ch % 13 - 6).double()
    assert (pre_g.abs() + s2.abs()).max().item() < X.TWO24
    assert (pre_b.abs() + s1.abs()).max().item() < X.TWO24
    gbuf = torch.full((C + 2 * G,), 7.0, **f)
    bbuf = torch.full((C + 2 * G,), -9.0, **f)
    gacc, bacc = gbuf[G:G + C], bbuf[G:G + C]
    gacc.copy_(pre_g.float())
    bacc.copy_(pre_b.float())
    _e().bn_bwd(k["dy"], None, k["x"], k["mean"], one, one, False, False,
                True, gacc, bacc)
    X.check_exact(gacc, pre_g + s2, "dgamma_acc")
    X.check_exact(bacc, pre_b + s1, "dbeta_acc")
    for buf, v in ((gbuf, 7.0), (bbuf, -9.0)):
        assert (buf[:G] == v).all() and (buf[G + C:] == v).all(), \
            "accumulator guard elements were written"
