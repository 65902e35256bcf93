"""gemm_bt_add: the bt GEMM with a bf16 [M, N] addend in its epilogue (GPU).

C = bf16(float(bf16(A @ B^T)) + float(R)): the accumulator is rounded to
bf16 first, then R is added in fp32 and the sum rounded again. That is the
composition gemm_bt followed by a bf16 add, so every check here is
bit-equality, never a tolerance.

Shapes: both tile configurations (128x128 for N % 128 == 0, else 256x64),
M below, at and above one and two tiles, and K = 1, 2, 3 and 5 K-tiles: the
parity of the tile count picks the staging buffer that receives R, and with
one tile R is staged before the loop."""
import pytest
import torch

from _mfma_exact_common import (ASYM3, PM1, PM12, check_budget, check_exact,
                                exact_ref_bt, ints, small_share)

pytestmark = pytest.mark.gpu

KS = [64, 128, 192, 320]
CASES = ([(m, n) for n in (128, 256) for m in (1, 127, 128, 129, 257)]
         + [(m, n) for n in (64, 192) for m in (255, 256, 257, 300)])


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
    return a, b, r


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mn", CASES)
def test_bit_equal_to_gemm_then_add(mn, k):
    e = _ext()
    m, n = mn
    a, b, r = _operands(m, n, k, 1000 * k + 7 * m + n)
    r0 = r.clone()
    got = e.gemm_bt_add(a, b, r)
    want = e.gemm_bt(a, b) + r
    assert got.dtype == torch.bfloat16 and got.shape == (m, n)
    assert torch.equal(got, want)
    assert torch.equal(r, r0)  # the addend is only read


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("mn", [(129, 128), (257, 256), (257, 64),
                                (300, 192)])
def test_sliced_addend_with_poisoned_neighbours(mn, k):
    """r is a 16-byte-aligned slice in the middle of a NaN-filled buffer:
    16 bytes of NaN before it, and NaN where the rows m >= M of the last
    tile (up to 255 of them) would lie. A tail row read past M and leaking
    into a stored row, or a wrong base, turns the output NaN."""
    e = _ext()
    m, n = mn
    a, b, r_vals = _operands(m, n, k, 31 * m + n + k)
    flat = torch.full((8 + m * n + 256 * n,), float("nan"), device="cuda",
                      dtype=torch.bfloat16)
    r = flat[8:8 + m * n].view(m, n)
    r.copy_(r_vals)
    assert r.data_ptr() % 16 == 0 and r.data_ptr() != flat.data_ptr()
    got = e.gemm_bt_add(a, b, r)
    assert torch.equal(got, e.gemm_bt(a, b) + r_vals)
    assert bool(torch.isnan(flat[:8]).all()) \
        and bool(torch.isnan(flat[8 + m * n:]).all())


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mn", [(257, 256), (300, 192)])
def test_exact_integers(mn, k):
    """Independent of gemm_bt: integer operands, fp64 CPU reference rounded
    to bf16 after the product and again after the add. With |A| = 1 and
    |B| <= 3 the products' sums have a standard deviation of sqrt(5.75 K)
    <= 43 at K = 320, so nearly all outputs are integers bf16 holds exactly
    and a +-1 error (a dropped k element, a neighbouring row's addend)
    cannot hide in a rounding."""
    m, n = mn
    gen = torch.Generator().manual_seed(5 * k + m)
    a = ints((m, k), PM1, gen)
    b = ints((n, k), ASYM3, gen)
    r = ints((m, n), PM12, gen)
    prod = exact_ref_bt(a, b)
    check_budget(prod, k, a.float(), b.float(), bf16_out=True)
    ref = prod.to(torch.bfloat16).double() + r.double()
    share = small_share(ref)
    assert share >= 0.9, ("share of |ref| <= 256 below 90%", share)
    got = _ext().gemm_bt_add(a.cuda(), b.cuda(), r.cuda())
    check_exact(got, ref, "gemm_bt_add %s K=%d" % (mn, k))


def test_refusals():
    e = _ext()
    m, n, k = 129, 128, 64
    a, b, r = _operands(m, n, k, 3)
    assert torch.equal(e.gemm_bt_add(a, b, r), e.gemm_bt(a, b) + r)
    with pytest.raises(RuntimeError, match="bf16"):
        e.gemm_bt_add(a, b, r.float())
    with pytest.raises(RuntimeError, match="shape"):
        e.gemm_bt_add(a, b, torch.zeros(m, n + 64, device="cuda",
                                        dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="shape"):
        e.gemm_bt_add(a, b, r[:-1])
    wide = torch.zeros(m, 2 * n, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.gemm_bt_add(a, b, wide[:, :n])
    flat = torch.zeros(m * n + 8, device="cuda", dtype=torch.bfloat16)
    odd = flat[1:1 + m * n].view(m, n)
    assert odd.is_contiguous() and odd.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError, match="aligned"):
        e.gemm_bt_add(a, b, odd)
    with pytest.raises(RuntimeError, match="device"):
        e.gemm_bt_add(a, b, r.cpu())
