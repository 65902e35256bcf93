"""Bit-exact integer tests of the MFMA kernels (gemm_bt.hip, gemm_tn.hip,
conv3x3.hip) against fp64 references, plus one real-valued case per kernel
family under a derived per-element bound.

Operands are small non-zero integers (tests/_mfma_exact_common.py): every
partial sum is exact in fp32 in any order, so fp32 outputs are bit-equal to
the fp64 reference and bf16 outputs to the reference rounded once. The
split-K routes, whose atomics fold in arrival order, become bit-checkable
too. The conv shapes are picked from conv3x3_pick_splitk so that both the
split-K and the non-split route of each tile shape run; the non-split route
is PROVEN per case through the stats return (None on split-K shapes).
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


def _cl(x):
    """CPU [N,C,H,W] -> channels_last GPU tensor."""
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _wvals(k):
    """Second operand's value set by reduction length: the richer set
    while >= 90% of |ref| stays <= 256 (sigma = sqrt(2.5 * 5.75 * k) = 91
    at k = 576), +-1 beyond (sigma = sqrt(2.5 * k) = 76 at k = 2304)."""
    return X.ASYM3 if k <= 640 else X.PM1


# ---- Part A: the GEMMs ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bt_case(M, N, K, stats=False):
    gen = _gen(1000 + M + 7 * N + 13 * K)
    a = X.ints((M, K), X.PM1 if stats else X.PM12, gen)
    b = X.ints((N, K), X.PM1 if stats else X.ASYM3, gen)
    ref = X.exact_ref_bt(a, b)
    X.check_budget(ref, K, a, b, bf16_out=True)
    return a.cuda(), b.cuda(), ref


_BT_M = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513]
# N = 128: 128x128 tile; N = 64, 192: 256x64 tile (192 = 3 n-tiles).
# Every M at K = 192 (odd tile count, last tile in buffer 0), every K at
# M = 257 (64 = single K tile), and one 27-tile grid (not a multiple of 8)
_BT_CASES = ([(m, n, 192) for n in (64, 128, 192) for m in _BT_M] +
             [(257, n, k) for n in (64, 128, 192) for k in (64, 128, 320)] +
             [(1025, 192, 192)])


@pytest.mark.parametrize("M,N,K", _BT_CASES)
def test_gemm_bt_exact(M, N, K):
    a, b, ref = _bt_case(M, N, K)
    X.check_exact(_e().gemm_bt(a, b), ref, f"gemm_bt {M}x{N}x{K}")


def _bt_tiles_m(M, N):
    return -(-M // (128 if N % 128 == 0 else 256))


def _consume_pooled(part, y2d):
    """Hand capped (pooled, atomically folded) partials to BN as the model
    does: bn_finalize reads them and stores zeros back."""
    C = y2d.shape[1]
    f = dict(device="cuda", dtype=torch.float32)
    _e().bn_fwd_train(y2d, torch.ones(C, **f), torch.zeros(C, **f),
                      torch.zeros(C, **f), torch.ones(C, **f), 0.1, 1e-5,
                      None, True, part)


def _check_stats(part, ref_rows, tiles_m, what):
    """part [min(tiles_m, 192), 2C] summed over rows == (sum y, sum y^2) of
    the bf16-rounded reference, exactly."""
    C = ref_rows.shape[1]
    s, q = X.ref_stats(ref_rows)
    assert part.dtype == torch.float32
    assert tuple(part.shape) == (min(tiles_m, 192), 2 * C), part.shape
    got = part.double().sum(0).cpu()  # integers below 2^24: exact
    assert torch.equal(got[:C], s), \
        (what, "sum y", (got[:C] != s).nonzero().flatten()[:8].tolist(),
         (got[:C] - s).abs().max().item())
    assert torch.equal(got[C:], q), \
        (what, "sum y^2", (got[C:] != q).nonzero().flatten()[:8].tolist(),
         (got[C:] - q).abs().max().item())


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("M", [1, 129, 257])
def test_gemm_bt_stats_exact(M, N):
    """Uncapped fold: one partial row per m-tile, plain stores. A clamped
    duplicate of a tail row counted in the stats moves the sums."""
    a, b, ref = _bt_case(M, N, 192, stats=True)
    c, part = _e().gemm_bt_stats(a, b)
    X.check_exact(c, ref, f"gemm_bt_stats {M}x{N}")
    assert part.shape[0] == _bt_tiles_m(M, N)
    _check_stats(part, ref, _bt_tiles_m(M, N), f"gemm_bt_stats {M}x{N}")


def test_gemm_bt_stats_capped_exact():
    """194 m-tiles > the 192-row cap: atomics into the pooled buffer. The
    raw binding returns the pool itself, cleaned only by bn_finalize, so
    each call's partials go through bn_fwd_train; call 2 is wrong if the
    pool came back dirty."""
    M, N, K = 193 * 128 + 1, 128, 64
    a, b, ref = _bt_case(M, N, K, stats=True)
    for it in range(2):
        c, part = _e().gemm_bt_stats(a, b)
        try:
            X.check_exact(c, ref, f"gemm_bt_stats capped call {it}")
            _check_stats(part, ref, _bt_tiles_m(M, N), f"capped call {it}")
            _consume_pooled(part, c)
            assert not part.any(), "bn_finalize left the pool dirty"
        finally:
            part.zero_()  # a failure must not poison the shared pool


@pytest.mark.parametrize("M,N,K,splitk", [
    # 128x128 tile (M >= 128 and N % 128 == 0)
    (129, 128, 320, 2), (129, 128, 320, 3), (129, 128, 320, 4),
    (256, 256, 128, 8), (129, 128, 320, 0),
    # 256x64 tile: N % 128 != 0, or M < 128 (includes M = 64 with N = 128)
    (100, 64, 320, 2), (100, 64, 320, 3), (100, 64, 320, 4),
    (64, 128, 128, 8), (100, 192, 320, 0), (129, 64, 192, 0),
])
def test_gemm_bt_splitk_exact(M, N, K, splitk):
    """K = 320 is 5 K tiles: splitk 2 and 3 do not divide them, 4 gives
    per = 2 and an EMPTY last slice (early return); K = 128 with splitk 8
    has more slices than tiles. Bit-equal despite the atomics."""
    a, b, ref = _bt_case(M, N, K)
    X.check_budget(ref, K, a, b, bf16_out=False)
    c = _e().gemm_bt_splitk(a, b, splitk)
    assert c.dtype == torch.float32
    X.check_exact(c, ref, f"gemm_bt_splitk {M}x{N}x{K} sk{splitk}")


@functools.lru_cache(maxsize=None)
def _tn_case(K, N1, N2):
    gen = _gen(2000 + K + 3 * N1 + 5 * N2)
    a = X.ints((K, N1), X.PM12, gen)
    b = X.ints((K, N2), X.ASYM3, gen)
    ref = X.exact_ref_tn(a, b)
    X.check_budget(ref, K, a, b, bf16_out=False)
    return a.cuda(), b.cuda(), ref


_TN_CFG = [(64, 64), (64, 256), (256, 64), (256, 256)]  # KW 4, 2, 2, 1
# every K at the automatic pick; K = 4100 gives each KW group more than one
# chunk and a tail; splitk 1, 3 and 999 (> nchunks, clamped by the binding)
_TN_CASES = ([(k, n1, n2, 0) for n1, n2 in _TN_CFG
              for k in (1, 63, 64, 65, 127, 129, 1000, 4100)] +
             [(k, n1, n2, sk) for n1, n2 in _TN_CFG
              for k, sk in ((65, 1), (1000, 3), (129, 999))])


@pytest.mark.parametrize("K,N1,N2,splitk", _TN_CASES)
def test_gemm_tn_splitk_exact(K, N1, N2, splitk):
    """A K tail is where a clamped duplicate row would be ADDED into the
    reduction (K = 65, 129: one row past a chunk)."""
    a, b, ref = _tn_case(K, N1, N2)
    c = _e().gemm_tn_splitk(a, b, splitk)
    assert c.dtype == torch.float32
    X.check_exact(c, ref, f"gemm_tn {K}x{N1}x{N2} sk{splitk}")


@pytest.mark.parametrize("N1,N2", _TN_CFG)
@pytest.mark.parametrize("K", [65, 129, 1000])
def test_gemm_tn_splitk_accumulates_into_out(K, N1, N2):
    a, b, ref = _tn_case(K, N1, N2)
    out = torch.full((N1, N2), 3.0, device="cuda")
    got = _e().gemm_tn_splitk(a, b, 0, out)
    assert got.data_ptr() == out.data_ptr()
    X.check_exact(out, ref + 3, f"gemm_tn out= {K}x{N1}x{N2}")


@functools.lru_cache(maxsize=None)
def _wgrad_case(n, ci, h, w, co, stride):
    gen = _gen(3000 + n + ci + 3 * h + 5 * w + 7 * co + stride)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = X.ints((n, ci, h, w), X.PM12, gen)
    dy = X.ints((n, co, ho, wo), X.ASYM3, gen)
    ref = X.exact_ref_conv_dw(x, (co, ci, 3, 3), dy, stride)  # [co,ci,3,3]
    X.check_budget(ref, n * ho * wo, x, dy, bf16_out=False)
    return _cl(x), _cl(dy), ref


# odd extents, M % 64 != 0 (198/30, 49/16, 512/128 rows), both tile widths
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 64, 9, 11, 64), (1, 128, 7, 7, 128),
                                   (2, 64, 16, 16, 128)])
def test_gemm_tn3x3_exact(shape, stride):
    """Gather wgrad vs fp64 conv2d_weight, four ways: flat dY; dY in its own
    zero-halo padded layout (the APAD row map); out= in [Cout,Cin,3,3]
    layout (the perm epilogue) and out= in the native 2-D layout, both
    accumulating onto a non-zero fill."""
    e = _e()
    n, ci, h, w, co = shape
    x, dy, ref = _wgrad_case(n, ci, h, w, co, stride)
    native = ref.permute(0, 2, 3, 1).reshape(co, 9 * ci)  # [Cout, 3,3,Cin]
    dy2d = X.rows(dy).contiguous()
    what = f"tn3x3 {shape} s{stride}"

    X.check_exact(e.gemm_tn3x3_splitk(dy2d, x, stride, 0), native,
                  what + " flat")
    xp, dyp = e.pad_nhwc(x), e.pad_nhwc(dy)
    X.check_exact(e.gemm_tn3x3_splitk_padded(dyp, xp, h, w, stride, 0),
                  native, what + " padded dy")
    out4 = torch.full((co, ci, 3, 3), 3.0, device="cuda")
    e.gemm_tn3x3_splitk(dy2d, x, stride, 0, out4)
    X.check_exact(out4, ref + 3, what + " out=[Cout,Cin,3,3]")
    out2 = torch.full((co, 9 * ci), 5.0, device="cuda")
    e.gemm_tn3x3_splitk_padded(dy2d, xp, h, w, stride, 0, out2)
    X.check_exact(out2, native + 5, what + " out= native")


@pytest.mark.parametrize("shape", [
    (4, 3, 32, 64, 2),    # stem conv0: Cin=3 (cpad->8), stride 2
    (4, 32, 32, 32, 1),   # stem conv1
    (4, 32, 64, 32, 1),   # stem conv2 (Cout=64, no dy pad)
])
def test_gemm_tn3x3_small_exact(shape):
    import torch.nn.functional as F

    n, ci, co, hw, stride = shape
    gen = _gen(3500 + ci + co)
    ho = (hw - 1) // stride + 1
    x = X.ints((n, ci, hw, hw), X.PM12, gen)
    dy = X.ints((n, co, ho, ho), X.ASYM3, gen)
    ref = X.exact_ref_conv_dw(x, (co, ci, 3, 3), dy, stride)
    X.check_budget(ref, n * ho * ho, x, dy, bf16_out=False)
    dy2d = X.rows(_cl(dy))
    if co < 64:
        dy2d = F.pad(dy2d, (0, 64 - co))
    cfull = _e().gemm_tn3x3_small(dy2d.contiguous(), _cl(x), stride)
    cinp = max(8, 1 << (ci - 1).bit_length())
    dw = cfull[:co, :9 * cinp].view(co, 3, 3, cinp).permute(0, 3, 1, 2)
    X.check_exact(dw[:, :ci].contiguous(), ref, f"tn3x3_small {shape}")
    # the padded channels and rows of the output are products with zeros
    assert not dw[:, ci:].any() and not cfull[co:, :9 * cinp].any()


@pytest.mark.parametrize("stride,shape", [(1, (2, 64, 9, 11)),
                                          (2, (1, 128, 7, 9))])
def test_conv3x3_wgrad_operand_exact(stride, shape):
    """shift9 operand [9*Cin, ceil64(M)] vs an independent fp64 gather
    (unfold): row (tap, c), column (n, oy, ox), zero past M."""
    import torch.nn.functional as F

    n, ci, h, w = shape
    x = X.ints(shape, X.ASYM3, _gen(3700 + stride))
    got = _e().conv3x3_wgrad_operand(_cl(x), stride).cpu()
    cols = F.unfold(x.double(), 3, padding=1, stride=stride)  # [n, ci*9, L]
    L = cols.shape[2]
    ref = (cols.view(n, ci, 9, L).permute(2, 1, 0, 3)
           .reshape(9 * ci, n * L))
    M = n * L
    assert tuple(got.shape) == (9 * ci, (M + 63) // 64 * 64)
    assert torch.equal(got[:, :M].double(), ref)
    assert not got[:, M:].any()


# ---- Part B: conv3x3 ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _conv_case(n, ci, h, w, co, stride, stats=False, half_zero=False):
    """x, w3 (as ops/conv.py builds it) and the fp64 reference rows. Stats
    cases use +-1 on both operands; half_zero blanks a fixed half of the
    input CHANNELS (never single elements: every tap stays non-zero)."""
    from edl_amd.ops.conv import _repack_w3

    gen = _gen(4000 + n + ci + 3 * h + 5 * w + 7 * co + stride)
    k = 9 * ci
    x = X.ints((n, ci, h, w), X.PM1 if stats else X.PM12, gen)
    if half_zero:
        x[:, 1::2] = 0
    wt = X.ints((co, ci, 3, 3), X.PM1 if stats else _wvals(k), gen)
    ref = X.rows(X.exact_ref_conv(x, wt, stride)).contiguous()
    X.check_budget(ref, k, x, wt, bf16_out=True)
    return _cl(x), _repack_w3(wt.cuda()), ref


def _pick_splitk(M, co, ci):
    """conv3x3_pick_splitk (conv3x3.hip), for the route comments/asserts."""
    bm, bn = (128, 128) if co % 128 == 0 else (256, 64)
    tiles = -(-M // bm) * (co // bn)
    kt = 9 * ci // 64
    if tiles >= 224 or kt < 8:
        return 1
    return max(1, min(384 // tiles, kt // 4))


# slices per (shape, stride 1 / 2), from _pick_splitk:
#   (2, 64, 9, 11, 64)     M 198 / 60    1 tile   -> 2 / 2   (KT 9: cap 2)
#   (2, 128, 14, 14, 256)  M 392 / 98    8 / 2    -> 4 / 4   (KT 18: cap 4)
#   (1, 256, 7, 7, 128)    M 49 / 16     1 tile   -> 9 / 9   (KT 36: cap 9)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,slices", [((2, 64, 9, 11, 64), 2),
                                          ((2, 128, 14, 14, 256), 4),
                                          ((1, 256, 7, 7, 128), 9)])
def test_conv3x3_fwd_splitk_exact(shape, slices, stride):
    """Split-K route: fp32 atomics into the pooled buffer, cast_bf16_zero.
    Two calls: the second is wrong if the pool came back dirty."""
    n, ci, h, w, co = shape
    x, w3, ref = _conv_case(n, ci, h, w, co, stride)
    assert _pick_splitk(ref.shape[0], co, ci) == slices
    y, part = _e().conv3x3_fwd_stats(x, w3, stride)
    assert part is None  # the split-K route folds no stats
    X.check_exact(y, ref, f"conv3x3 split {shape} s{stride} call 0")
    X.check_exact(_e().conv3x3_fwd(x, w3, stride), ref,
                  f"conv3x3 split {shape} s{stride} call 1")


_NONSPLIT = {
    # Cout 256: 128x128 tile, 98 m-tiles x 2 = 196 tiles, UNCAPPED stats
    # (plain stores into [98, 512]); M = 12482 ends inside the last tile
    "c256-s1": ((2, 64, 79, 79, 256), 1, False),
    "c256-s2": ((2, 64, 158, 157, 256), 2, False),
    # Cout 128: 128x128 tile, 196 m-tiles, capped (atomic) stats
    "c128-capped": ((2, 64, 112, 112, 128), 1, True),
    # Cout 64: 256x64 tile, 196 m-tiles, capped stats
    "c64-capped": ((4, 64, 112, 112, 64), 1, True),
}


@pytest.mark.parametrize("name", list(_NONSPLIT))
def test_conv3x3_fwd_nonsplit_exact(name):
    """Non-split route of each tile shape: direct bf16 epilogue + the stats
    fold. The route is asserted through the stats return."""
    shape, stride, capped = _NONSPLIT[name]
    n, ci, h, w, co = shape
    x, w3, ref = _conv_case(n, ci, h, w, co, stride, stats=True,
                            half_zero=capped)
    M = ref.shape[0]
    tiles_m = -(-M // (128 if co % 128 == 0 else 256))
    assert (tiles_m > 192) == capped
    for it in range(2 if capped else 1):
        y, part = _e().conv3x3_fwd_stats(x, w3, stride)
        assert part is not None, "shape fell back to the split-K route"
        try:
            X.check_exact(y, ref, f"conv3x3 non-split {name} call {it}")
            _check_stats(part, ref, tiles_m, f"{name} call {it}")
            if capped:
                _consume_pooled(part, y)
                assert not part.any(), "bn_finalize left the pool dirty"
        finally:
            if capped:
                part.zero_()  # a failure must not poison the shared pool
    if name == "c256-s1":  # the *_padded twin on the pad_nhwc buffer
        y, part = _e().conv3x3_fwd_stats_padded(_e().pad_nhwc(x), w3, stride,
                                                h, w)
        assert part is not None
        X.check_exact(y, ref, "conv3x3 non-split padded twin")
        _check_stats(part, ref, tiles_m, "padded twin")


@pytest.mark.parametrize("shape", [
    # dgrad = the forward kernel on dy with Cin <-> Cout swapped:
    # dy [2,128,12,12] -> Cout_dgrad 64: 256x64 tile, 2 tiles, KT 18:
    # split-K, 4 slices
    (2, 64, 12, 12, 128),
    # forward non-split (196 tiles); dgrad on dy [2,256,79,79] ->
    # Cout_dgrad 64: 256x64 tile, 49 tiles, KT 36: split-K, 7 slices
    (2, 64, 79, 79, 256),
])
def test_conv3x3_s1_backward_exact(shape):
    """Conv2dFast stride-1 backward: x.grad bit-equal to fp64 conv2d_input
    rounded once to bf16; the fp32 weight grad (gather wgrad) bit-equal."""
    from edl_amd.ops.conv import Conv2dFast

    n, ci, h, w, co = shape
    gen = _gen(5000 + co)
    x = X.ints((n, ci, h, w), X.PM1, gen)
    wt = X.ints((co, ci, 3, 3), X.PM12, gen)
    dy = X.ints((n, co, h, w), X.PM1, gen)
    dx_ref = X.exact_ref_conv_dx((n, ci, h, w), wt, dy, 1)
    X.check_budget(dx_ref, 9 * co, dy, wt, bf16_out=True)
    dw_ref = X.exact_ref_conv_dw(x, (co, ci, 3, 3), dy, 1)
    X.check_budget(dw_ref, n * h * w, x, dy, bf16_out=False)
    assert _pick_splitk(n * h * w, ci, co) == (4 if co == 128 else 7)

    conv = Conv2dFast(ci, co, 3, padding=1, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(wt.float())
    xg = _cl(x).requires_grad_(True)
    y = conv(xg)
    y.backward(_cl(dy))
    X.check_exact(xg.grad.contiguous(), dx_ref, f"s1 dgrad {shape}")
    assert conv.weight.grad.dtype == torch.float32
    X.check_exact(conv.weight.grad.contiguous(), dw_ref, f"wgrad {shape}")


# the four shapes of test_conv3x3_s2_dgrad_numerics at N = 1: the parity
# classes depend on H, W alone (14, 28 even; 13 odd) and the launch split
# on Cin % 128 (128, 256, 512 vs 64)
@pytest.mark.parametrize("shape", [(1, 128, 128, 14), (1, 256, 256, 28),
                                   (1, 512, 512, 14), (1, 64, 128, 13)])
def test_conv3x3_s2_dgrad_exact(shape):
    from edl_amd.ops.conv import _repack_w3_s2dgrad

    n, ci, co, hw = shape
    gen = _gen(6000 + ci + co + hw)
    ho = (hw + 1) // 2
    wt = X.ints((co, ci, 3, 3), X.PM1, gen)
    dy = X.ints((n, co, ho, ho), X.PM12, gen)
    ref = X.exact_ref_conv_dx((n, ci, hw, hw), wt, dy, 2)
    X.check_budget(ref, 4 * co, dy, wt, bf16_out=True)  # <= 4 taps / class
    dx2d = _e().conv3x3s2_dgrad(_cl(dy), _repack_w3_s2dgrad(wt.cuda()),
                                hw, hw)
    X.check_exact(dx2d, X.rows(ref).contiguous(), f"s2 dgrad {shape}")


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("shape", [
    (2, 3, 32, 2, 64),    # stem conv0: Cin 3 padded to 8, cpt 16, stride 2
    (2, 32, 32, 1, 33),   # stem conv1: odd HW
    (2, 32, 64, 1, 28),   # stem conv2
])
def test_conv3x3_small_fwd_exact(shape, stats):
    from edl_amd.ops.conv import _repack_w3_small, _small_cpt

    n, ci, co, stride, hw = shape
    gen = _gen(7000 + ci + co)
    x = X.ints((n, ci, hw, hw), X.PM12, gen)
    wt = X.ints((co, ci, 3, 3), X.ASYM3, gen)
    ref = X.rows(X.exact_ref_conv(x, wt, stride)).contiguous()
    X.check_budget(ref, 9 * ci, x, wt, bf16_out=True)
    cpt = _small_cpt(ci)
    w3s = _repack_w3_small(wt.cuda(), cpt)
    if not stats:
        y = _e().conv3x3_small_fwd(_cl(x), w3s, co, cpt, stride)
        X.check_exact(y, ref, f"conv3x3_small {shape}")
        return
    y, part = _e().conv3x3_small_fwd_stats(_cl(x), w3s, co, cpt, stride)
    X.check_exact(y, ref, f"conv3x3_small stats {shape}")
    tiles_m = -(-ref.shape[0] // 256)  # kSmallBM; uncapped: plain stores
    assert tiles_m <= 192
    _check_stats(part, ref, tiles_m, f"conv3x3_small {shape}")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cpg", [16, 64])
def test_conv3x3_grouped_fwd_exact(cpg, stride):
    """cpg 16: block-diagonal repack (gw 64); cpg 64: per-group dense."""
    from edl_amd.ops.conv import _repack_w3_grouped

    C = 2 * max(cpg, 32)  # 64 channels / 4 groups, 128 channels / 2 groups
    gen = _gen(8000 + cpg + stride)
    x = X.ints((1, C, 7, 9), X.PM12, gen)
    wt = X.ints((C, cpg, 3, 3), X.ASYM3, gen)
    ref = X.rows(X.exact_ref_conv(x, wt, stride, groups=C // cpg))
    X.check_budget(ref, 9 * cpg, x, wt, bf16_out=True)
    y = _e().conv3x3_grouped_fwd(_cl(x), _repack_w3_grouped(wt.cuda()),
                                 stride)
    X.check_exact(y, ref.contiguous(), f"grouped cpg{cpg} s{stride}")


# ---- Part C: one real-valued case per family, derived per-element bound ----

def _report(name, ratio):
    print(f"\nmfma-exact err/bound {name}: {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)


def test_gemm_bt_real_valued_bound():
    """Integers never round inside the accumulator; randn operands do.
    |err| <= 2^-8 (|ref| + E) + E with E = 2 K 2^-24 (|A| |B|^T)."""
    M, N, K = 257, 128, 320
    torch.manual_seed(0)
    a = (torch.randn(M, K, device="cuda") * 2).to(torch.bfloat16)
    b = (torch.randn(N, K, device="cuda") +
         torch.arange(K, device="cuda") * 0.01).to(torch.bfloat16)
    c = _e().gemm_bt(a, b)
    _report("gemm_bt 257x128x320", X.bound_ratio(
        c, X.exact_ref_bt(a, b), X.exact_ref_bt(a.abs(), b.abs()), K))


def test_gemm_tn_real_valued_bound():
    K, N1, N2 = 1000, 128, 128
    torch.manual_seed(2)
    a = (torch.randn(K, N1, device="cuda") * 1.5).to(torch.bfloat16)
    b = (torch.randn(K, N2, device="cuda") +
         torch.arange(N2, device="cuda") * 0.003).to(torch.bfloat16)
    c = _e().gemm_tn_splitk(a, b, 0)
    _report("gemm_tn_splitk 1000x128x128", X.bound_ratio(
        c, X.exact_ref_tn(a, b), X.exact_ref_tn(a.abs(), b.abs()), K))


def test_conv3x3_real_valued_bound():
    from edl_amd.ops.conv import Conv2dFast, _repack_w3

    n, ci, h, w, co = 2, 64, 79, 79, 256
    torch.manual_seed(0)
    wt = Conv2dFast(ci, co, 3, padding=1, bias=False).weight.detach().to(
        torch.bfloat16)  # the default init, as test_conv3x3_fwd_numerics
    x = (torch.randn(n, ci, h, w, device="cuda") * 1.5).to(torch.bfloat16)
    y, part = _e().conv3x3_fwd_stats(_cl(x), _repack_w3(wt.cuda()), 1)
    assert part is not None  # the non-split route
    _report("conv3x3_fwd 2x64x79x79->256", X.bound_ratio(
        y, X.rows(X.exact_ref_conv(x, wt, 1)),
        X.rows(X.exact_ref_conv(x.abs(), wt.abs(), 1)), 9 * ci))
