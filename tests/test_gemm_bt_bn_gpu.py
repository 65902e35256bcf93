"""gemm_bt_bn: the bt GEMM with the eval BN(+Add)+ReLU apply in its epilogue.

    yb = bf16(acc); v = fmaf(float(yb), scale[n], shift[n]); v += float(R)
    with a residual; v = fmaxf(v, 0) with relu; C = bf16(v)

That is gemm_bt followed by bn_fwd_eval (bnrelu.hip apply_octet), so the
checks against that pair are bit-equality, never a tolerance. One further
check is independent of both kernels: integer operands, an fp64 CPU
reference and a derived per-element bound.

Shapes: both tile configurations (128x128 for N % 128 == 0, else 256x64; N
192 has three n-tiles, so a per-tile scale offset shows), M below, at and
above one and two tiles, and K = 1, 2, 3 and 5 K-tiles: the parity of the
tile count picks the staging buffer that receives the residual, and with
one tile it is staged before the loop."""
import itertools

import pytest
import torch

from _eval_affine_common import affine as _affine, affine_bound_ratio
from _mfma_exact_common import ASYM3, PM1, check_budget, exact_ref_bt, ints, \
    small_share

pytestmark = pytest.mark.gpu

KS = [64, 128, 192, 320]
CASES = ([(m, n) for n in (128, 256) for m in (1, 127, 128, 129, 257)]
         + [(m, n) for n in (64, 192) for m in (255, 256, 257, 300)])
VARIANTS = list(itertools.product((False, True), (False, True)))  # relu, res


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ext():
    from edl_amd import ops

    return ops.ext()


def _operands(m, n, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(m, k, device="cuda", generator=g).to(torch.bfloat16)
    b = torch.randn(n, k, device="cuda", generator=g).to(torch.bfloat16)
    r = (torch.randn(m, n, device="cuda", generator=g) * 4).to(torch.bfloat16)
    scale, shift = _affine(n, g)
    return a, b, scale, shift, r


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mn", CASES)
def test_bit_equal_to_gemm_then_bn(mn, k):
    e = _ext()
    m, n = mn
    ops = _operands(m, n, k, 1000 * k + 7 * m + n)
    a, b, scale, shift, r = ops
    before = [t.clone() for t in ops]
    y = e.gemm_bt(a, b)
    for relu, with_res in VARIANTS:
        res = r if with_res else None
        got = e.gemm_bt_bn(a, b, scale, shift, relu, res)
        want = e.bn_fwd_eval(y, scale, shift, res, relu)
        assert got.dtype == torch.bfloat16 and got.shape == (m, n)
        assert torch.equal(got, want), (relu, with_res)
    for t, t0 in zip(ops, before):  # every operand is only read
        assert torch.equal(t, t0)


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("mn", [(129, 128), (257, 256), (257, 64),
                                (300, 192)])
def test_poisoned_neighbours(mn, k):
    """res is a 16-byte-aligned slice in the middle of a NaN-filled buffer
    (NaN before it, and NaN where the rows m >= M of the last tile would
    lie); scale and shift are slices of NaN buffers with NaN directly before
    and after their N values. A read past either end that reaches a stored
    element turns the output NaN."""
    e = _ext()
    m, n = mn
    a, b, scale_v, shift_v, r_vals = _operands(m, n, k, 31 * m + n + k)
    flat = torch.full((8 + m * n + 256 * n,), float("nan"), device="cuda",
                      dtype=torch.bfloat16)
    r = flat[8:8 + m * n].view(m, n)
    r.copy_(r_vals)
    assert r.data_ptr() % 16 == 0 and r.data_ptr() != flat.data_ptr()
    sflat = torch.full((2, n + 8), float("nan"), device="cuda")
    scale, shift = sflat[0, 3:3 + n], sflat[1, 5:5 + n]
    scale.copy_(scale_v)
    shift.copy_(shift_v)
    assert scale.is_contiguous() and shift.is_contiguous()
    y = e.gemm_bt(a, b)
    for relu, with_res in VARIANTS:
        got = e.gemm_bt_bn(a, b, scale, shift, relu, r if with_res else None)
        assert not bool(torch.isnan(got).any()), (relu, with_res)
        assert torch.equal(got, e.bn_fwd_eval(
            y, scale_v, shift_v, r_vals if with_res else None, relu))
    assert bool(torch.isnan(flat[:8]).all()) \
        and bool(torch.isnan(flat[8 + m * n:]).all())
    assert int(torch.isnan(sflat).sum()) == 16


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mn", [(257, 256), (300, 192)])
def test_exact_reference(mn, k):
    """Independent of gemm_bt and bn_fwd_eval: integer A (+-1) and B
    ({-3, -1, 2, 3}), so the product is exact in any order and yb is the
    fp64 product rounded once to bf16; real-valued scale, shift and res."""
    m, n = mn
    gen = torch.Generator().manual_seed(5 * k + m)
    a = ints((m, k), PM1, gen)
    b = ints((n, k), ASYM3, gen)
    prod = exact_ref_bt(a, b)
    check_budget(prod, k, a.float(), b.float(), bf16_out=True)
    assert small_share(prod) >= 0.9
    yb = prod.to(torch.bfloat16).double()
    g = torch.Generator(device="cuda").manual_seed(k + n)
    scale, shift = _affine(n, g)
    r = (torch.randn(m, n, device="cuda", generator=g) * 4).to(torch.bfloat16)
    worst = 0.0
    for relu, with_res in VARIANTS:
        got = _ext().gemm_bt_bn(a.cuda(), b.cuda(), scale, shift, relu,
                                r if with_res else None)
        r64 = r.double().cpu() if with_res else torch.zeros(m, n,
                                                            dtype=torch.float64)
        ratio = affine_bound_ratio(got, yb, scale, shift, r64, relu)
        print(f"\ngemm_bt_bn err/bound {mn} K={k} relu={relu} "
              f"res={with_res}: {ratio:.4f}")
        worst = max(worst, ratio)
    assert worst <= 1.0, worst


def test_refusals():
    e = _ext()
    m, n, k = 129, 128, 64
    a, b, scale, shift, r = _operands(m, n, k, 3)
    y = e.gemm_bt(a, b)
    assert torch.equal(e.gemm_bt_bn(a, b, scale, shift, True, r),
                       e.bn_fwd_eval(y, scale, shift, r, True))
    assert torch.equal(e.gemm_bt_bn(a, b, scale, shift, False),
                       e.bn_fwd_eval(y, scale, shift, None, False))
    # a and b: the checks of gemm_bt
    with pytest.raises(RuntimeError, match="bf16"):
        e.gemm_bt_bn(a.float(), b, scale, shift, True)
    with pytest.raises(RuntimeError, match="% 64"):
        e.gemm_bt_bn(a[:, :32], b[:, :32], scale, shift, True)
    # scale / shift
    with pytest.raises(RuntimeError, match="fp32"):
        e.gemm_bt_bn(a, b, scale.double(), shift, True)
    with pytest.raises(RuntimeError, match="fp32"):
        e.gemm_bt_bn(a, b, scale, shift.to(torch.bfloat16), True)
    with pytest.raises(RuntimeError, match="shape"):
        e.gemm_bt_bn(a, b, scale[:-1], shift, True)
    with pytest.raises(RuntimeError, match="shape"):
        e.gemm_bt_bn(a, b, scale, torch.cat([shift, shift]), True)
    with pytest.raises(RuntimeError, match="shape"):
        e.gemm_bt_bn(a, b, scale.view(1, n), shift, True)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.gemm_bt_bn(a, b, torch.cat([scale, scale])[::2], shift, True)
    with pytest.raises(RuntimeError, match="device"):
        e.gemm_bt_bn(a, b, scale.cpu(), shift, True)
    with pytest.raises(RuntimeError, match="device"):
        e.gemm_bt_bn(a, b, scale, shift.cpu(), True)
    # res: the refusals of gemm_bt_add
    with pytest.raises(RuntimeError, match="bf16"):
        e.gemm_bt_bn(a, b, scale, shift, True, r.float())
    with pytest.raises(RuntimeError, match="shape"):
        e.gemm_bt_bn(a, b, scale, shift, True,
                     torch.zeros(m, n + 64, device="cuda",
                                 dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="shape"):
        e.gemm_bt_bn(a, b, scale, shift, True, r[:-1])
    wide = torch.zeros(m, 2 * n, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.gemm_bt_bn(a, b, scale, shift, True, wide[:, :n])
    flat = torch.zeros(m * n + 8, device="cuda", dtype=torch.bfloat16)
    odd = flat[1:1 + m * n].view(m, n)
    assert odd.is_contiguous() and odd.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError, match="aligned"):
        e.gemm_bt_bn(a, b, scale, shift, True, odd)
    with pytest.raises(RuntimeError, match="device"):
        e.gemm_bt_bn(a, b, scale, shift, True, r.cpu())
