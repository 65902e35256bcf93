"""The elementwise half of bnrelu.hip (bn_apply_kernel, bn_apply_pad_kernel,
bn_bwd_dx_kernel, bn_bwd_dx_pad_kernel, phase 2 of bn_bwd_fused_kernel)
against fp64 CPU references computed from the bf16 inputs, and the operand
checks of the three bindings (idiom of _mfma_exact_common.py: conditions are
asserted on the REFERENCE before the kernel's output is looked at, every
measured ratio is printed before it is asserted).

These kernels are index arithmetic plus about ten flops, so a bug is the
wrong channel's scale, a mask bit one place off, or a row/octet split that
is wrong for one width class. The operands below make every one of those
move a value by at least one bf16 ulp.

1. Eval apply, bit-exact. x in {-3,-1,2,3}, scale[c] cycling through
   {1,-2,.5,2,-1,-.5}, shift[c] = c % 5 - 2, res in {-2,-1,1,2}: x * scale +
   shift is a multiple of 1/2 of magnitude <= 8, and so is the sum with res
   (<= 10): the fma and the add are exact in fp32 and the result is a bf16
   value (20 half-steps need 5 of its 8 bits). y is bit-equal to the
   reference for every (relu, add).

2. Training forward, y within a derived bound, mask exact. Integer x in
   -3..3 keeps sum x and sum x^2 exact in fp32 in any order. With u = 2^-24
   per rounding and r = mean^2 / var: 1/M, sum * (1/M) and the fma leave
   mean within 2u and var within (3 + 7r)u; var + eps adds u, rsqrtf halves
   it and adds 1 ulp <= 2u: invstd within (4 + 3.5r)u, scale = g * invstd
   within (5 + 3.5r)u, scale * mean within (8 + 3.5r)u, shift = beta - that
   one more of |shift| <= |beta| + |scale mean|, the apply's fma one more of
   its result. Per magnitude, in units of 2^-23: |x scale| 3 + 1.75r, |beta|
   1, |scale mean| 5 + 1.75r, all <= 6 for r <= 0.5 (asserted on the
   reference): the y_bound of test_bn_finalize_gpu.py,
       6 * 2^-23 * (|x scale| + |beta| + |scale mean|) + 2^-8 |y|,
   carries over to an M that is no power of two. The residual add rounds
   once more, u of (that sum + |res|), res itself being exact:
       7 * 2^-23 * (|x scale| + |beta| + |scale mean| + |res|) + 2^-8 |y|.
   The mask byte is taken from the fp32 value and a positive fp32 never
   rounds to bf16 zero, so unpack(mask) == (y > 0) exactly, and == (pre > 0)
   wherever the reference pre-activation is farther from 0 than the bound
   (asserted to be at least 90% of the elements).

3. Backward, bit-exact tier. M a power of two (1/M exact), dy and x in
   {-3,-1,2,3}, mean[c] = c % 3 - 1, invstd[c] in {.5,1,2}, gamma[c] in
   {1,-2,.5,4}, random mask bytes. Every intermediate of dx_octet (xhat,
   s1, s2, s1/M, xhat*s2, that /M, both differences, gamma*invstd) is
   asserted to be an fp32 value, so whatever the compiler contracts into
   fmas, dx rounds exactly once, to bf16: dx, dres bit-equal, dgamma and
   dbeta exact. All eight (relu, add, training) instantiations, both padded
   ones and the four fused single-launch ones (whose LDS-atomic fold is
   exact on integers too).

4. Backward, bounded tier (any M): the same integers, so s1 and s2 stay
   exact and only the dx arithmetic rounds. Roundings: 1/M and the product
   (2u of a = s1/M), xhat*s2 and its scaling (3u of b = xhat s2/M), g - a
   (u of |g| + |a|), - b (u of |g| + |a| + |b|), gamma*invstd and the last
   product (2u of everything). Per magnitude: |g| 4, |a| 6, |b| 6 (8 with
   the two roundings of a real-valued xhat) <= 8:
       2^-8 |dx| + 8 * 2^-24 * |gamma invstd| (|g| + |s1|/M + |xhat s2|/M).
   One real-valued case adds the accumulation errors E1, E2 of the two sums
   as test_bn_wide_gpu.py derives them ((M + 8) u sum|term|).

5. Refusals: every spoiled operand is at least as large in bytes as the
   right one (wider dtype, more rows, [2C], a non-contiguous view of a
   buffer of the same or a larger size, a CPU tensor), except the short
   mask the binding refused before.

docs/kernels.md ("bnrelu.hip") records the measured maxima and which case
reaches which template instantiation.
"""
import functools

import pytest
import torch

import _mfma_exact_common as X

pytestmark = pytest.mark.gpu

EPS32 = float(torch.tensor(1e-5, dtype=torch.float32).double())
U = 2.0 ** -24
BF16 = torch.bfloat16

VARIANTS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.fixture(autouse=True)
def _gpu(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    # the shipped routes, whatever the caller's environment says
    monkeypatch.setenv("EDL_BN_SLAB", "1")
    monkeypatch.setenv("EDL_BN_BWD_FUSED", "0")


def _e():
    from edl_amd import ops
    return ops.ext()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _is_f32(v64):
    return torch.equal(v64.float().double(), v64)


def _cuda(t):
    return None if t is None else t.cuda()


W8 = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128])  # bit k = channel 8o + k


def _unpack(mask):
    """[M, C/8] mask bytes -> bool [M, C]."""
    return ((mask.cpu().long().unsqueeze(-1) & W8) != 0).flatten(1)


def _poison(numel):
    """Allocate, NaN-fill and free a buffer of the padded size, so that
    recycled storage would show in a halo the kernel failed to write."""
    junk = torch.full((numel,), float("nan"), device="cuda", dtype=BF16)
    del junk


def _split_padded(xp, nhw):
    """Padded [N, H+2, W+2, C] -> interior rows [M, C]; asserts the shape
    and that the halo is exactly zero (NaN != 0, so NaN fails too)."""
    n, h, w = nhw
    assert tuple(xp.shape[:3]) == (n, h + 2, w + 2), xp.shape
    halo = xp.clone()
    halo[:, 1:-1, 1:-1, :] = 0
    assert bool((halo == 0).all().item()), "halo is not zero"
    return xp[:, 1:-1, 1:-1, :].reshape(n * h * w, xp.shape[3])


def _ratio(got, ref, bound):
    """max(err / bound); 0 where the result is exact (a bound can be 0)."""
    err = (got.detach().cpu().double() - ref).abs()
    return torch.where(err > 0, err / bound.clamp(min=1e-300),
                       torch.zeros_like(err)).max().item()


# ---------------- 1. eval apply, bit-exact ----------------

CAP = 2048 * 256  # octets of one pass of the capped grid (elementwise_grid)
# (M, C) -> (full grid-stride passes, octets of the last one)
EVAL_SHAPES = {
    (1, 8): (0, 1),             # one thread
    (37, 24): (0, 111),         # C/8 = 3: the % and / branch of OctSplit
    (300, 40): (0, 1500),       # C/8 = 5, partial last block (5*256 + 220)
    (129, 2048): (0, 33024),
    (5, 4104): (0, 2565),       # wide and no power of two (C/8 = 513)
    (21846, 192): (1, 16),      # C/8 = 24; a second pass of 16 octets
    ((1 << 17) + 3, 64): (2, 24),  # pow2; two passes and a tail
}


@functools.lru_cache(maxsize=None)
def _eval_case(M, C):
    gen = _gen(3000 + 5 * M + C)
    x = X.ints((M, C), X.ASYM3, gen)
    res = X.ints((M, C), X.PM12, gen)
    ch = torch.arange(C)
    scale = torch.tensor([1, -2, 0.5, 2, -1, -0.5])[ch % 6]
    shift = (ch % 5 - 2).float()
    pre = x.double() * scale.double() + shift.double()
    refs = {}
    for add in (False, True):
        p = pre + res.double() if add else pre
        assert torch.equal(p.to(BF16).double(), p), "reference is not bf16"
        assert p.abs().max().item() <= 10
        if p.numel() >= 4096:  # both sides of the ReLU, and its edge
            pos = (p > 0).double().mean().item()
            zero = (p == 0).double().mean().item()
            assert 0.3 < pos < 0.7 and zero > 0.02, (pos, zero)
        refs[add] = p
    return dict(x=x.cuda(), res=res.cuda(), scale=scale.cuda(),
                shift=shift.cuda(), refs=refs)


def test_eval_shapes_pass_the_grid_cap():
    for (M, C), want in EVAL_SHAPES.items():
        assert divmod(M * (C // 8), CAP) == want, (M, C)


@pytest.mark.parametrize("M,C", list(EVAL_SHAPES))
def test_eval_apply_exact(M, C):
    k = _eval_case(M, C)
    for relu, add in VARIANTS:
        y = _e().bn_fwd_eval(k["x"], k["scale"], k["shift"],
                             k["res"] if add else None, relu)
        ref = k["refs"][add]
        X.check_exact(y, ref.clamp(min=0) if relu else ref,
                      f"eval y M={M} C={C} relu={relu} add={add}")


# ---------------- 2. training forward ----------------

TRAIN_SHAPES = [(37, 8), (300, 64), (129, 2048),
                (4 * 256 // (256 // 8) + 1, 256)]  # 4 blocks + one row
TRAIN_PADDED = [(2, 7, 9, 64), (3, 5, 5, 256)]


@functools.lru_cache(maxsize=None)
def _train_case(M, C):
    gen = _gen(5000 + 7 * M + C)
    xi = torch.randint(-3, 4, (M, C), generator=gen)
    flat = (xi == xi[0]).all(0)  # a constant channel has var = 0
    xi[0, flat] = (xi[0, flat] + 4) % 7 - 3  # the next value of {-3..3}
    x = xi.to(BF16)
    res = X.ints((M, C), X.PM12, gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen)
    xd, g, b, rd = x.double(), gamma.double(), beta.double(), res.double()
    assert xd.abs().sum(0).max().item() < X.TWO24, "sum|x| budget"
    assert (xd * xd).sum(0).max().item() < X.TWO24, "sum x^2 budget"
    mean = xd.sum(0) / M
    var = (xd * xd).sum(0) / M - mean * mean
    assert var.min().item() > 0, "degenerate case: var <= 0"
    assert (mean * mean / var).max().item() <= 0.5, "r = mean^2/var budget"
    scale = g * (var + EPS32).rsqrt()
    pre0 = xd * scale + (b - scale * mean)
    mag0 = xd.abs() * scale + b.abs() + scale * mean.abs()
    refs = {}
    for relu, add in VARIANTS:
        pre = pre0 + rd if add else pre0
        mag = mag0 + rd.abs() if add else mag0
        y = pre.clamp(min=0) if relu else pre
        bound = 2.0 ** -8 * y.abs() + (7 if add else 6) * 2.0 ** -23 * mag
        sure = pre.abs() > bound
        assert sure.double().mean().item() >= 0.9, "mask check covers little"
        refs[relu, add] = dict(y=y, bound=bound, pos=pre > 0, sure=sure)
    return dict(x=x, res=res, gamma=gamma, beta=beta, refs=refs)


def _run_train(k, relu, add, pad_hw):
    C = k["gamma"].numel()
    f = dict(device="cuda", dtype=torch.float32)
    return _e().bn_fwd_train(
        k["x"].cuda(), k["gamma"].cuda(), k["beta"].cuda(),
        torch.zeros(C, **f), torch.ones(C, **f), 0.1, 1e-5,
        k["res"].cuda() if add else None, relu, None, pad_hw)


def _check_train(tag, ref, y, mask, relu, M, C):
    ratio = _ratio(y, ref["y"], ref["bound"])
    print(f"train fwd {tag}: y err/bound {ratio:.4f}")
    assert ratio <= 1.0, ratio
    if not relu:
        assert mask.numel() == 0
        return
    assert tuple(mask.shape) == (M, C // 8) and mask.dtype == torch.uint8
    bits = _unpack(mask)
    assert torch.equal(bits, y.cpu() > 0), \
        f"{int((bits != (y.cpu() > 0)).sum())} mask bits differ from y > 0"
    wrong = (bits != ref["pos"]) & ref["sure"]
    assert not wrong.any(), f"{int(wrong.sum())} mask bits differ from pre > 0"


@pytest.mark.parametrize("relu,add", VARIANTS)
@pytest.mark.parametrize("M,C", TRAIN_SHAPES)
def test_train_forward(M, C, relu, add):
    k = _train_case(M, C)
    y, _, _, mask = _run_train(k, relu, add, None)
    assert y.dtype == BF16 and tuple(y.shape) == (M, C)
    _check_train(f"M={M} C={C} relu={relu} add={add}", k["refs"][relu, add],
                 y, mask, relu, M, C)


@pytest.mark.parametrize("N,H,W,C", TRAIN_PADDED)
def test_train_forward_padded(N, H, W, C):
    M = N * H * W
    k = _train_case(M, C)
    _poison(N * (H + 2) * (W + 2) * C)
    yp, _, _, mask = _run_train(k, True, False, (H, W))
    assert yp.dtype == BF16 and yp.shape[3] == C
    y = _split_padded(yp, (N, H, W))
    _check_train(f"padded {(N, H, W, C)}", k["refs"][True, False], y, mask,
                 True, M, C)


@pytest.mark.parametrize("pad", [False, True])
def test_train_mask_at_exact_zero(pad):
    """The edge of the ReLU: rows come in (x, -x) pairs, so every channel
    sums to 0, mean is exactly 0 and, with beta = 0, shift = 0 - scale * 0
    is +0: the pre-activation is fl(x * scale), which has the sign of x and
    is +0 where x = 0. The mask bit of a zero must be clear (`>`, not
    `>=`), through bn_apply_kernel and bn_apply_pad_kernel."""
    N, H, W, C = 2, 4, 4, 64
    M = N * H * W
    gen = _gen(41)
    half = torch.randint(-3, 4, (M // 2, C), generator=gen)
    xi = torch.stack([half, -half], 1).view(M, C)
    assert (xi.sum(0) == 0).all() and (xi * xi).sum(0).min().item() > 0
    zero = (xi == 0).double().mean().item()
    assert 0.1 <= zero <= 0.2, zero
    gamma = torch.rand(C, generator=gen) + 0.5
    k = dict(x=xi.to(BF16), gamma=gamma, beta=torch.zeros(C), res=None)
    if pad:
        _poison(N * (H + 2) * (W + 2) * C)
    y, mean, _, mask = _run_train(k, True, False, (H, W) if pad else None)
    if pad:
        y = _split_padded(y, (N, H, W))
    assert not mean.any(), "mean is not exactly 0"
    assert tuple(mask.shape) == (M, C // 8) and mask.dtype == torch.uint8
    bits = _unpack(mask)
    assert torch.equal(bits, xi > 0), \
        f"{int((bits != (xi > 0)).sum())} mask bits differ from x > 0"
    assert torch.equal(y.cpu() > 0, xi > 0) and not y.cpu()[xi <= 0].any()


# ---------------- 3 / 4. backward dx, dres ----------------

@functools.lru_cache(maxsize=None)
def _bwd_case(M, C):
    gen = _gen(8000 + 3 * M + C)
    dy = X.ints((M, C), X.ASYM3, gen)
    x = X.ints((M, C), X.ASYM3, gen)
    mask = torch.randint(256, (M, C // 8), generator=gen, dtype=torch.uint8)
    ch = torch.arange(C)
    mean = (ch % 3 - 1).float()
    invstd = torch.tensor([0.5, 1, 2])[ch % 3]
    gamma = torch.tensor([1, -2, 0.5, 4])[ch % 4]
    return dict(dy=dy, x=x, mask=mask, mean=mean, invstd=invstd, gamma=gamma)


def _ref_bwd(k, relu, training, sum_errors=False):
    """fp64 backward of the operands k. `exact`: every fp32 intermediate of
    the kernel's expression is an fp32 value (decided on the reference).
    `bound`: section 4 of the docstring; sum_errors adds the accumulation
    errors E1, E2 of real-valued sums."""
    g = k["dy"].double()
    if relu:
        g = g * _unpack(k["mask"]).double()
    M = g.shape[0]
    mean, istd = k["mean"].double(), k["invstd"].double()
    d = k["x"].double() - mean
    xhat = d * istd
    t = g * xhat
    s1, s2 = g.sum(0), t.sum(0)
    kk = k["gamma"].double() * istd
    e1 = (M + 8) * U * g.abs().sum(0) if sum_errors else torch.zeros_like(s1)
    e2 = (M + 8) * U * t.abs().sum(0) if sum_errors else torch.zeros_like(s2)
    if training:
        inv_m = torch.tensor(1.0 / M, dtype=torch.float64)
        a, p = s1 * inv_m, xhat * s2
        b = p * inv_m
        t1 = g - a
        t2 = t1 - b
        dx = kk * t2
        inter = (d, xhat, t, s1, s2, inv_m, a, p, b, t1, t2, kk, dx)
    else:
        dx = kk * g
        inter = (d, xhat, t, s1, s2, kk, dx)
    exact = (all(_is_f32(v) for v in inter)
             and g.abs().sum(0).max().item() < X.TWO24
             and t.abs().sum(0).max().item() < X.TWO24)
    bound = (2.0 ** -8 * dx.abs() + kk.abs() * (e1 + xhat.abs() * e2) / M
             + 8 * U * kk.abs() * (g.abs() + s1.abs() / M
                                   + (xhat * s2).abs() / M))
    return dict(g=g, dx=dx, dgamma=s2, dbeta=s1, exact=exact, bound=bound,
                dgamma_bound=e2, dbeta_bound=e1)


@functools.lru_cache(maxsize=None)
def _int_ref(M, C, relu, training):
    return _ref_bwd(_bwd_case(M, C), relu, training)


def _run_bwd(k, relu, add, training, pad_hw=None, accs=(None, None), dy=None):
    return _e().bn_bwd(
        k["dy"].cuda() if dy is None else dy,
        k["mask"].cuda() if relu else None, k["x"].cuda(), k["mean"].cuda(),
        k["invstd"].cuda(), k["gamma"].cuda(), relu, add, training, accs[0],
        accs[1], pad_hw)


def _check_bwd_exact(what, ref, outs, add, nhw=None):
    dx, dgamma, dbeta, dres = outs
    if nhw is not None:
        dx = _split_padded(dx, nhw)
    X.check_exact(dx, ref["dx"], "dx " + what)
    X.check_exact(dgamma, ref["dgamma"], "dgamma " + what)
    X.check_exact(dbeta, ref["dbeta"], "dbeta " + what)
    if add:
        X.check_exact(dres, ref["g"], "dres " + what)


BWD_EXACT = [(32, 8), (64, 8), (256, 64), (4096, 256), (512, 2048)]
BWD_ALL = [(r, a, t) for r, a in VARIANTS for t in (True, False)]
BWD_EXACT_CASES = ([(M, C) + v for M, C in BWD_EXACT for v in BWD_ALL] +
                   # two grid-stride passes (1048576 octets, cap 524288)
                   [(1 << 17, 64, True, True, True),
                    (1 << 17, 64, False, False, False)])


@pytest.mark.parametrize("M,C,relu,add,training", BWD_EXACT_CASES)
def test_bwd_dx_exact(M, C, relu, add, training):
    assert M & (M - 1) == 0
    ref = _int_ref(M, C, relu, training)
    assert ref["exact"], "an intermediate of the reference is no fp32 value"
    share = (ref["dx"].to(BF16).double() == ref["dx"]).double().mean().item()
    what = f"M={M} C={C} relu={relu} add={add} training={training}"
    print(f"bwd exact {what}: {share:.3f} of dx are bf16 values unrounded")
    outs = _run_bwd(_bwd_case(M, C), relu, add, training)
    assert outs[0].dtype == BF16
    _check_bwd_exact(what, ref, outs, add)


def test_noncontiguous_dy_is_copied():
    M, C = 64, 8
    k = _bwd_case(M, C)
    dy = torch.empty(C, M, device="cuda", dtype=BF16).t()
    dy.copy_(k["dy"])
    assert not dy.is_contiguous()
    _check_bwd_exact("strided dy", _int_ref(M, C, True, True),
                     _run_bwd(k, True, True, True, dy=dy), True)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N,H,W,C", [(2, 4, 4, 64), (4, 2, 8, 8),
                                     (1, 16, 8, 128)])
def test_bwd_dx_padded_exact(N, H, W, C, relu):
    M = N * H * W
    assert M & (M - 1) == 0
    ref = _int_ref(M, C, relu, True)
    assert ref["exact"], "an intermediate of the reference is no fp32 value"
    _poison(N * (H + 2) * (W + 2) * C)
    outs = _run_bwd(_bwd_case(M, C), relu, False, True, (H, W))
    _check_bwd_exact(f"padded {(N, H, W, C)} relu={relu}", ref, outs, False,
                     (N, H, W))


# (M, C, finalizer blocks = clamp(2C / 256, 1, 8))
FUSED = [(4096, 64, 1), (512, 2048, 8)]


@pytest.mark.parametrize("relu,add", VARIANTS)
@pytest.mark.parametrize("M,C,nfin", FUSED)
def test_bwd_fused_exact(M, C, nfin, relu, add, monkeypatch):
    """EDL_BN_BWD_FUSED=1: reduce, finalize and dx in one launch. Its
    row-only LDS-atomic fold is exact on integers, so the outputs are
    bit-equal to the reference, not merely close to the unfused ones; the
    second call runs on the workspace the first one reset."""
    assert min(max(2 * C // 256, 1), 8) == nfin
    ref = _int_ref(M, C, relu, True)
    assert ref["exact"], "an intermediate of the reference is no fp32 value"
    monkeypatch.setenv("EDL_BN_BWD_FUSED", "1")
    for call in range(2):
        outs = _run_bwd(_bwd_case(M, C), relu, add, True)
        _check_bwd_exact(f"fused M={M} C={C} relu={relu} add={add} "
                         f"call={call}", ref, outs, add)


def test_bwd_fused_accumulators(monkeypatch):
    """Direct-grad accumulators of the single-launch kernel (eight
    finalizer blocks, each a slice of [dbeta; dgamma]): preset + sum, and
    nothing outside [C] written."""
    M, C, G = 512, 2048, 8
    ref = _int_ref(M, C, True, True)
    assert ref["exact"]
    f = dict(device="cuda", dtype=torch.float32)
    ch = torch.arange(C)
    pre_g, pre_b = (ch % 11 - 5).double(), (ch % 13 - 6).double()
    assert (pre_g.abs() + ref["dgamma"].abs()).max().item() < X.TWO24
    assert (pre_b.abs() + ref["dbeta"].abs()).max().item() < X.TWO24
    gbuf = torch.full((C + 2 * G,), 7.0, **f)
    bbuf = torch.full((C + 2 * G,), -9.0, **f)
    gacc, bacc = gbuf[G:G + C], bbuf[G:G + C]
    gacc.copy_(pre_g.float())
    bacc.copy_(pre_b.float())
    monkeypatch.setenv("EDL_BN_BWD_FUSED", "1")
    outs = _run_bwd(_bwd_case(M, C), True, False, True, accs=(gacc, bacc))
    _check_bwd_exact("fused with accumulators", ref, outs, False)
    X.check_exact(gacc, pre_g + ref["dgamma"], "dgamma_acc")
    X.check_exact(bacc, pre_b + ref["dbeta"], "dbeta_acc")
    for buf, v in ((gbuf, 7.0), (bbuf, -9.0)):
        assert (buf[:G] == v).all() and (buf[G + C:] == v).all(), \
            "accumulator guard elements were written"


def _check_bwd_bounded(what, ref, outs, add, nhw=None):
    dx, dgamma, dbeta, dres = outs
    if nhw is not None:
        dx = _split_padded(dx, nhw)
    ratio = _ratio(dx, ref["dx"], ref["bound"])
    print(f"bwd bounded {what}: dx err/bound {ratio:.4f}")
    assert ratio <= 1.0, ratio
    X.check_exact(dgamma, ref["dgamma"], "dgamma " + what)
    X.check_exact(dbeta, ref["dbeta"], "dbeta " + what)
    if add:
        X.check_exact(dres, ref["g"], "dres " + what)


@pytest.mark.parametrize("relu,add", VARIANTS)
@pytest.mark.parametrize("M,C", [(1, 8), (37, 8), (300, 64), (129, 1024)])
def test_bwd_dx_bounded(M, C, relu, add):
    ref = _int_ref(M, C, relu, True)
    outs = _run_bwd(_bwd_case(M, C), relu, add, True)
    _check_bwd_bounded(f"M={M} C={C} relu={relu} add={add}", ref, outs, add)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N,H,W,C", TRAIN_PADDED)
def test_bwd_dx_padded_bounded(N, H, W, C, relu):
    M = N * H * W
    ref = _int_ref(M, C, relu, True)
    _poison(N * (H + 2) * (W + 2) * C)
    outs = _run_bwd(_bwd_case(M, C), relu, False, True, (H, W))
    _check_bwd_bounded(f"padded {(N, H, W, C)} relu={relu}", ref, outs, False,
                       (N, H, W))


def test_bwd_real_valued():
    """randn operands, statistics of x itself: the full bound, with the
    accumulation errors of the two sums."""
    M, C = 300, 256
    gen = _gen(99)
    x = torch.randn(M, C, generator=gen).to(BF16)
    xd = x.double()
    k = dict(dy=torch.randn(M, C, generator=gen).to(BF16), x=x,
             mask=torch.randint(256, (M, C // 8), generator=gen,
                                dtype=torch.uint8),
             mean=xd.mean(0).float(),
             invstd=(xd.var(0, unbiased=False) + EPS32).rsqrt().float(),
             gamma=torch.rand(C, generator=gen) + 0.5)
    ref = _ref_bwd(k, True, True, sum_errors=True)
    dx, dgamma, dbeta, _ = _run_bwd(k, True, False, True)
    ratios = dict(dx=_ratio(dx, ref["dx"], ref["bound"]),
                  dgamma=_ratio(dgamma, ref["dgamma"], ref["dgamma_bound"]),
                  dbeta=_ratio(dbeta, ref["dbeta"], ref["dbeta_bound"]))
    print("bwd real M=300 C=256 relu: err/bound",
          " ".join(f"{n} {v:.4f}" for n, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


# ---------------- 5. the bindings refuse what the kernels cannot index ----

RM, RC = 4, 64


def _wide(t):
    return t.to({BF16: torch.float32, torch.float32: torch.float64,
                 torch.uint8: torch.int16}[t.dtype])


def _strided(t):
    """Same shape, values and device, not contiguous, in a buffer of the
    same size (2-D: transposed) or twice the size (1-D: every other one)."""
    if t.dim() == 2:
        v = torch.empty_like(t.t().contiguous()).t()
    else:
        v = torch.empty(2 * t.numel(), device=t.device, dtype=t.dtype)[::2]
    v.copy_(t)
    assert v.shape == t.shape and not v.is_contiguous()
    return v


SPOIL = {
    "wide": _wide,
    "cpu": lambda t: t.cpu(),
    "strided": _strided,
    "rows": lambda t: torch.cat([t, t[:1]]),      # [M + 1, C]
    "2C": lambda t: torch.cat([t, t], -1),        # [2C], or [M, 2C]
    "short": lambda t: t[1:],                     # the mask only
}

REFUSALS = [
    ("train", "x", "wide", "bf16"), ("train", "x", "cpu", "GPU"),
    ("train", "x", "strided", "contiguous"),
    ("train", "x", "2C", r"\[M, C\]"),
    ("train", "gamma", "wide", "gamma must be fp32"),
    ("train", "gamma", "2C", r"\[M, C\]"),
    ("train", "beta", "2C", "beta must be fp32"),
    ("train", "beta", "cpu", "beta must be fp32"),
    ("train", "rmean", "wide", "running_mean must be fp32"),
    ("train", "rvar", "strided", "running_var must be fp32"),
    ("train", "res", "wide", "res must be bf16"),
    ("train", "res", "rows", "res must be bf16"),
    ("train", "res", "strided", "res must be bf16"),
    ("train", "res", "cpu", "res must be bf16"),
    ("eval", "x", "wide", "bf16"), ("eval", "x", "cpu", "GPU"),
    ("eval", "x", "strided", "contiguous"), ("eval", "x", "2C", r"\[M, C\]"),
    ("eval", "scale", "wide", "scale must be fp32"),
    ("eval", "shift", "2C", "shift must be fp32"),
    ("eval", "shift", "strided", "shift must be fp32"),
    ("eval", "shift", "cpu", "shift must be fp32"),
    ("eval", "res", "wide", "res must be bf16"),
    ("eval", "res", "rows", "res must be bf16"),
    ("eval", "res", "strided", "res must be bf16"),
    ("eval", "res", "cpu", "res must be bf16"),
    ("bwd", "x", "wide", "bf16"), ("bwd", "x", "cpu", "GPU"),
    ("bwd", "x", "strided", "contiguous"), ("bwd", "x", "2C", r"\[M, C\]"),
    ("bwd", "dy", "wide", "dy must be bf16"),
    ("bwd", "dy", "rows", "dy must be bf16"),
    ("bwd", "dy", "cpu", "dy must be bf16"),
    ("bwd", "mean", "2C", "mean must be fp32"),
    ("bwd", "mean", "cpu", "mean must be fp32"),
    ("bwd", "invstd", "wide", "invstd must be fp32"),
    ("bwd", "invstd", "strided", "invstd must be fp32"),
    ("bwd", "gamma", "wide", "gamma must be fp32"),
    ("bwd", "mask", "wide", "relu path needs the fwd mask"),
    ("bwd", "mask", "strided", "relu path needs the fwd mask"),
    ("bwd", "mask", "cpu", "relu path needs the fwd mask"),
    ("bwd", "mask", "short", "relu path needs the fwd mask"),
]


def _refusal_call(entry, a):
    e = _e()
    if entry == "train":
        return e.bn_fwd_train(a["x"], a["gamma"], a["beta"], a["rmean"],
                              a["rvar"], 0.1, 1e-5, a["res"], True, None)
    if entry == "eval":
        return e.bn_fwd_eval(a["x"], a["scale"], a["shift"], a["res"], True)
    return e.bn_bwd(a["dy"], a["mask"], a["x"], a["mean"], a["invstd"],
                    a["gamma"], True, False, True)


def _refusal_operands():
    x = torch.zeros(RM, RC, device="cuda", dtype=BF16)
    one = torch.ones(RC, device="cuda")
    a = dict(x=x, dy=x.clone(), res=x.clone(),
             mask=torch.zeros(RM, RC // 8, device="cuda", dtype=torch.uint8))
    for name in ("gamma", "beta", "rmean", "rvar", "scale", "shift", "mean",
                 "invstd"):
        a[name] = one.clone()
    return a


@pytest.mark.parametrize("entry", ["train", "eval", "bwd"])
def test_unspoiled_operands_are_accepted(entry):
    _refusal_call(entry, _refusal_operands())
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry,name,spoil,match", REFUSALS)
def test_refusals(entry, name, spoil, match):
    a = _refusal_operands()
    good = a[name]
    a[name] = SPOIL[spoil](good)
    if spoil != "short":  # a missing check could not read past an allocation
        assert (a[name].numel() * a[name].element_size()
                >= good.numel() * good.element_size())
    with pytest.raises(RuntimeError, match=match):
        _refusal_call(entry, a)
