"""Zero-halo padded-layout hand-offs around the bottleneck 3x3 convs (GPU).

The 3x3 implicit-GEMM kernels read a padded [N, H+2, W+2, C] image. These
tests cover the three ways the per-consumer pad_nhwc copies are avoided:
the *_padded bindings (pad once, keep it), bn_fwd_train(pad_hw=) writing
the conv's padded input, and bn_bwd(pad_hw=) writing the conv's padded dy
that dgrad and the gather wgrad read.

Shapes: N=2 with (C,H,W) in (64,5,5), (128,6,7), (64,7,6) — M=50 is below
one 64-row K chunk (wgrad K-tail), odd/non-square sizes exercise stride 2,
C=128 selects the 128-wide tile configuration."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 2
SHAPES = [(64, 5, 5), (128, 6, 7), (64, 7, 6)]
STRIDES = [1, 2]  # every shape has an odd H or W, so all run stride 2


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ext():
    from edl_amd import ops

    return ops.ext()


def _interior(xp):
    from edl_amd.ops.conv import padded_interior

    return padded_interior(xp)


def _out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def _stats_part(x2d):
    """BN stats partials [1, 2C] (sums, then sums of squares), the form a
    producing conv's epilogue hands over as pre_part."""
    xf = x2d.float()
    return torch.cat([xf.sum(0), xf.square().sum(0)]).view(1, -1).contiguous()


def _bn_fwd(x2d, c, pad_hw, pre_part=None):
    """bn_fwd_train on fresh running stats -> (outs, rmean, rvar, gamma)."""
    g = torch.Generator(device="cuda").manual_seed(7)
    gamma = torch.rand(c, device="cuda", generator=g) + 0.5
    beta = torch.randn(c, device="cuda", generator=g) * 0.2
    rm = torch.zeros(c, device="cuda")
    rv = torch.ones(c, device="cuda")
    outs = _ext().bn_fwd_train(x2d, gamma, beta, rm, rv, 0.1, 1e-5, None, True,
                               pre_part, pad_hw)
    return outs, rm, rv, gamma


def _poison(numel):
    """Allocate, NaN-fill and free a buffer of the padded size, so that
    recycled storage would show in a halo the kernel failed to write."""
    junk = torch.full((numel,), float("nan"), device="cuda",
                      dtype=torch.bfloat16)
    del junk


def _halo_is_zero(xp):
    halo = xp.clone()
    halo[:, 1:-1, 1:-1, :] = 0
    return bool((halo == 0).all().item())  # NaN != 0, so NaN fails too


def _conv_kslices(m, c):
    """K slices the 3x3 forward kernel runs at [m, c] x [c, 9c]
    (conv3x3.hip conv3x3_pick_splitk)."""
    bm, bn = (128, 128) if c % 128 == 0 else (256, 64)
    tiles = -(-m // bm) * (c // bn)
    kt = 9 * c // 64
    if tiles >= 224 or kt < 8:
        return 1
    return max(1, min(384 // tiles, kt // 4))


def _assert_same_conv_result(got, ref, m, c):
    """Same kernel, same launch, same padded bytes (asserted by the
    caller): bit-equal — as long as the launch is deterministic. With more
    than two K slices the kernel folds fp32 partials with atomics in
    arrival order, and two runs of ONE call already differ; there the
    outputs may sit one bf16 rounding (2^-8 relative) apart, on top of a
    fp32-reorder absolute error far below the 1e-3 allowed."""
    if _conv_kslices(m, c) <= 2:  # x + y == y + x: two slices are exact
        assert torch.equal(got, ref)
    else:
        assert torch.allclose(got.float(), ref.float(), rtol=2 ** -7,
                              atol=1e-3), \
            (got.float() - ref.float()).abs().max().item()


def _padded_pair(c, h, w, seed):
    """(xp, x): a BN-written padded activation and the same values as an
    ordinary channels_last tensor (from the unpadded call, bit-equal)."""
    torch.manual_seed(seed)
    x2d = (torch.randn(N * h * w, c, device="cuda") * 2 + 0.3).to(
        torch.bfloat16)
    part = _stats_part(x2d)  # shared, see test_bn_fwd_train_pad_hw
    _poison(N * (h + 2) * (w + 2) * c)
    (xp, _, _, _), _, _, _ = _bn_fwd(x2d, c, (h, w), part)
    (y2d, _, _, _), _, _, _ = _bn_fwd(x2d, c, None, part)
    x = y2d.view(N, h, w, c).permute(0, 3, 1, 2)
    return xp, x


def _padded_dy(c, ho, wo, seed):
    """(dyp, dy): a BN-backward-written padded gradient and its interior
    as a contiguous channels_last tensor (same values by construction)."""
    e = _ext()
    torch.manual_seed(seed)
    m = N * ho * wo
    x2d = torch.randn(m, c, device="cuda").to(torch.bfloat16)
    g2d = torch.randn(m, c, device="cuda").to(torch.bfloat16)
    (_, mean, invstd, msk), _, _, gamma = _bn_fwd(x2d, c, None)
    _poison(N * (ho + 2) * (wo + 2) * c)
    dyp = e.bn_bwd(g2d, msk, x2d, mean, invstd, gamma, True, False, True,
                   None, None, (ho, wo))[0]
    ref = e.bn_bwd(g2d, msk, x2d, mean, invstd, gamma, True, False, True)[0]
    assert dyp.shape == (N, ho + 2, wo + 2, c)
    assert _halo_is_zero(dyp)
    got = _interior(dyp).permute(0, 2, 3, 1).reshape(m, c)
    # same fp32 expression in both kernels, rounded to bf16: allow one
    # bf16 ulp (2^-8 relative) for a differently contracted multiply-add
    assert torch.allclose(got.float(), ref.float(), rtol=2 ** -7, atol=1e-6)
    dy = _interior(dyp).contiguous(memory_format=torch.channels_last)
    return dyp, dy


@pytest.mark.parametrize("chw", SHAPES)
def test_bn_fwd_train_pad_hw(chw):
    """Interior, mask and statistics bit-equal to the unpadded call; halo
    exactly zero on recycled NaN storage; twice under the same conditions.

    Both calls get the SAME stats partials (pre_part), as in the model,
    where the producing conv's epilogue supplies them. The in-call stats
    kernel folds rows with LDS float atomics in arrival order, so two
    identical UNPADDED calls already differ in the last bits of invstd;
    that route is covered below with the reorder-sized tolerance."""
    c, h, w = chw
    torch.manual_seed(11)
    m = N * h * w
    x2d = (torch.randn(m, c, device="cuda") * 2 + 0.3).to(torch.bfloat16)
    part = _stats_part(x2d)
    (y, mean, invstd, msk), rm, rv, _ = _bn_fwd(x2d, c, None, part)
    for _ in range(2):
        _poison(N * (h + 2) * (w + 2) * c)
        (yp, mean_p, invstd_p, msk_p), rm_p, rv_p, _ = _bn_fwd(
            x2d, c, (h, w), part)
        assert yp.shape == (N, h + 2, w + 2, c) and yp.is_contiguous()
        assert _halo_is_zero(yp)
        assert torch.equal(yp[:, 1:-1, 1:-1, :].reshape(m, c), y)
        assert torch.equal(msk_p, msk)
        assert torch.equal(mean_p, mean) and torch.equal(invstd_p, invstd)
        assert torch.equal(rm_p, rm) and torch.equal(rv_p, rv)
        del yp
    # stats computed inside the call: sums of <= 100 fp32 terms in a
    # varying order (relative 1e-5 is ~100 * 2^-24 with margin), and y
    # within one bf16 ulp of the shared-partials result
    _poison(N * (h + 2) * (w + 2) * c)
    (yp, mean_p, invstd_p, _), _, _, _ = _bn_fwd(x2d, c, (h, w))
    assert _halo_is_zero(yp)
    assert torch.allclose(mean_p, mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(invstd_p, invstd, rtol=1e-5, atol=1e-6)
    assert torch.allclose(yp[:, 1:-1, 1:-1, :].reshape(m, c).float(),
                          y.float(), rtol=2 ** -7, atol=1e-3)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("chw", SHAPES)
def test_conv_fwd_from_bn_written_xp(chw, stride):
    """3x3 forward (with and without the stats epilogue) from a BN-written
    padded buffer is bit-equal to conv3x3_fwd on the plain tensor."""
    e = _ext()
    c, h, w = chw
    xp, x = _padded_pair(c, h, w, 21)
    w3 = (torch.randn(c, 9 * c, device="cuda") * 0.05).to(torch.bfloat16)
    # the bytes the kernel reads are the ones today's path pads up
    assert torch.equal(e.pad_nhwc(x), xp)
    ho, wo = _out_hw(h, w, stride)
    m = N * ho * wo
    ref = e.conv3x3_fwd(x, w3, stride)
    assert ref.shape == (m, c)
    _assert_same_conv_result(e.conv3x3_fwd_padded(xp, w3, stride, h, w), ref,
                             m, c)
    y_s, part_s = e.conv3x3_fwd_stats_padded(xp, w3, stride, h, w)
    y_r, part_r = e.conv3x3_fwd_stats(x, w3, stride)
    _assert_same_conv_result(y_s, ref, m, c)
    assert (part_s is None) == (part_r is None)
    if part_s is not None:
        assert torch.equal(part_s, part_r)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("chw", SHAPES)
def test_dgrad_from_padded_dy(chw, stride):
    """Stride-1 and stride-2 dgrad reading the BN-backward-written padded
    dy is bit-equal to today's pad-inside path on the same values."""
    e = _ext()
    c, h, w = chw
    ho, wo = _out_hw(h, w, stride)
    dyp, dy = _padded_dy(c, ho, wo, 31)
    wd = (torch.randn(c, 9 * c, device="cuda") * 0.05).to(torch.bfloat16)
    assert torch.equal(e.pad_nhwc(dy), dyp)
    if stride == 1:
        got = e.conv3x3_fwd_padded(dyp, wd, 1, ho, wo)
        ref = e.conv3x3_fwd(dy, wd, 1)
        _assert_same_conv_result(got, ref, N * h * w, c)
    else:  # the parity kernel has no K split: always bit-equal
        got = e.conv3x3s2_dgrad_padded(dyp, wd, h, w)
        ref = e.conv3x3s2_dgrad(dy, wd, h, w)
        assert torch.equal(got, ref)
    assert got.shape == (N * h * w, c)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("chw", SHAPES)
def test_wgrad_from_padded_xp_and_dy(chw, stride):
    """Gather wgrad from padded xp and padded dy (A-operand row map, K
    tail included) against today's binding and against fp32 torch, plus
    the out= accumulate layouts of direct-grad mode."""
    e = _ext()
    c, h, w = chw
    ho, wo = _out_hw(h, w, stride)
    xp, x = _padded_pair(c, h, w, 41)
    dyp, dy = _padded_dy(c, ho, wo, 42)
    dy2d = dy.permute(0, 2, 3, 1).reshape(-1, c)

    ref_tn = e.gemm_tn3x3_splitk(dy2d, x, stride, 0)
    ref_fp32 = torch.nn.grad.conv2d_weight(
        x.float(), (c, c, 3, 3), dy.float(), stride=(stride, stride),
        padding=(1, 1))

    def check(got3, off=0.0):
        assert got3.shape == (c, 9 * c)
        assert torch.allclose(got3, ref_tn + off, atol=0.5, rtol=0.02), \
            (got3 - ref_tn - off).abs().max().item()
        got4 = got3.view(c, 3, 3, c).permute(0, 3, 1, 2)
        assert torch.allclose(got4, ref_fp32 + off, atol=2.0, rtol=0.05), \
            (got4 - ref_fp32 - off).abs().max().item()

    # padded xp with the flat dy, then with the padded dy
    check(e.gemm_tn3x3_splitk_padded(dy2d, xp, h, w, stride, 0))
    check(e.gemm_tn3x3_splitk_padded(dyp, xp, h, w, stride, 0))
    # direct-grad accumulate: s-major [Cout, 9*Cin] (channels-last bucket)
    out2 = torch.full((c, 9 * c), 0.25, device="cuda")
    e.gemm_tn3x3_splitk_padded(dyp, xp, h, w, stride, 0, out2)
    check(out2, 0.25)
    # ... and the conv-weight [Cout, Cin, 3, 3] layout (epilogue remap)
    out4 = torch.full((c, c, 3, 3), 0.25, device="cuda")
    e.gemm_tn3x3_splitk_padded(dyp, xp, h, w, stride, 0, out4)
    check(out4.permute(0, 2, 3, 1).reshape(c, 9 * c), 0.25)
    # the deep-route operand from the padded buffer
    assert torch.equal(e.conv3x3_wgrad_operand_padded(xp, h, w, stride),
                       e.conv3x3_wgrad_operand(x, stride))


# ---- module wiring ----


class _Spy:
    """Counts calls of the extension's entry points by name."""

    def __init__(self, monkeypatch, names):
        self.calls = {n: 0 for n in names}
        e = _ext()
        for n in names:
            monkeypatch.setattr(e, n, self._wrap(n, getattr(e, n)))

    def _wrap(self, name, fn):
        def f(*a, **k):
            self.calls[name] += 1
            return fn(*a, **k)

        return f

    def reset(self):
        for n in self.calls:
            self.calls[n] = 0


_SPIED = ["pad_nhwc", "conv3x3_fwd", "conv3x3_fwd_padded",
          "conv3x3_fwd_stats", "conv3x3_fwd_stats_padded", "conv3x3s2_dgrad",
          "conv3x3s2_dgrad_padded", "gemm_tn3x3_splitk",
          "gemm_tn3x3_splitk_padded"]


def _make_blocks(c, stride):
    import edl_amd.ops.conv as conv_mod
    from edl_amd.models.resnet_vd import BottleneckVd

    torch.manual_seed(32)
    b1 = BottleneckVd(c, c, stride=stride, if_first=True).cuda().train()
    for mod in b1.modules():
        if isinstance(mod, conv_mod.Conv2dFast):
            mod.to(torch.bfloat16)
    return b1, copy.deepcopy(b1)


def _input(c, h, w, seed=33):
    torch.manual_seed(seed)
    x = torch.randn(N, c, h, w, device="cuda").to(torch.bfloat16)
    return x.contiguous(memory_format=torch.channels_last)


def _set_stages(monkeypatch, on):
    import edl_amd.ops.conv as conv_mod

    for flag in ("_PAD_ONCE", "_BN_PAD_OUT", "_BN_PAD_DX"):
        monkeypatch.setattr(conv_mod, flag, on)


def _assert_step_matches(y1, x1, b1, y2, x2, b2):
    assert torch.allclose(y1.float(), y2.float(), atol=1e-2, rtol=1e-2)
    assert torch.allclose(x1.grad.float(), x2.grad.float(), atol=1e-2,
                          rtol=1e-2)
    for p1, p2 in zip(b1.parameters(), b2.parameters()):
        assert (p1.grad is None) == (p2.grad is None)
        if p1.grad is not None:
            assert torch.allclose(p1.grad.float(), p2.grad.float(),
                                  atol=5e-2, rtol=5e-2), p1.shape


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("chw", SHAPES)
def test_bottleneck_step_fused_vs_optout(chw, stride, monkeypatch):
    """One BottleneckVd training step with the padded hand-offs wired
    against all three stages switched off; the fused step must not pad."""
    c, h, w = chw
    b1, b2 = _make_blocks(c, stride)
    x1 = _input(c, h, w).requires_grad_(True)
    x2 = x1.detach().clone().requires_grad_(True)
    spy = _Spy(monkeypatch, _SPIED)

    _set_stages(monkeypatch, True)
    y1 = b1(x1)
    y1.float().square().mean().backward()
    # forward from the BN-written buffer, dgrad and wgrad from the
    # BN-backward-written one: no pad anywhere
    assert spy.calls["pad_nhwc"] == 0
    assert spy.calls["conv3x3_fwd_stats_padded"] == 1
    assert spy.calls["gemm_tn3x3_splitk_padded"] == 1
    assert spy.calls["conv3x3_fwd"] == spy.calls["conv3x3s2_dgrad"] == 0
    assert (spy.calls["conv3x3_fwd_padded"]
            + spy.calls["conv3x3s2_dgrad_padded"]) == 1

    spy.reset()
    _set_stages(monkeypatch, False)
    y2 = b2(x2)
    y2.float().square().mean().backward()
    assert spy.calls["conv3x3_fwd_stats"] == 1
    assert spy.calls["gemm_tn3x3_splitk"] == 1
    assert spy.calls["conv3x3_fwd_stats_padded"] == 0

    _assert_step_matches(y1, x1, b1, y2, x2, b2)


def _two_consumer_loss(b, x):
    """The bottleneck's conv0 -> conv1 chain with the 3x3 conv's output
    given a second consumer, so autograd SUMS two gradients for it."""
    y0 = b.conv0(x, pad_out=b.conv1.conv.takes_padded())
    conv, bn = b.conv1.conv, b.conv1.bn
    c = conv(y0, bn_stats=True, dx_pad=True)
    y1 = bn(c, partials=conv.pop_bn_part(), dx_pad=conv.pop_dy_pad())
    return y1, y1.float().square().mean() + 0.5 * c.float().mean()


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("chw", SHAPES)
def test_summed_gradient_falls_back_to_pad(chw, stride, monkeypatch):
    """dy that is not the BN-written buffer's interior (here: a sum) must
    take the padding dgrad/wgrad path, and still match the opt-out run."""
    c, h, w = chw
    b1, b2 = _make_blocks(c, stride)
    x1 = _input(c, h, w).requires_grad_(True)
    x2 = x1.detach().clone().requires_grad_(True)
    spy = _Spy(monkeypatch, _SPIED)

    _set_stages(monkeypatch, True)
    y1, loss1 = _two_consumer_loss(b1, x1)
    loss1.backward()
    # dgrad padded dy itself (the unsuffixed bindings); wgrad still reads
    # the saved padded x, with the flat dy
    assert (spy.calls["conv3x3_fwd"] + spy.calls["conv3x3s2_dgrad"]) == 1
    assert (spy.calls["conv3x3_fwd_padded"]
            + spy.calls["conv3x3s2_dgrad_padded"]) == 0
    assert spy.calls["gemm_tn3x3_splitk_padded"] == 1

    _set_stages(monkeypatch, False)
    y2, loss2 = _two_consumer_loss(b2, x2)
    loss2.backward()
    _assert_step_matches(y1, x1, b1, y2, x2, b2)


@pytest.mark.parametrize("chw", SHAPES[:2])
def test_graph_capture_replay(chw, monkeypatch):
    """Forward+backward captured in a graph and replayed three times with
    new input: the halos are rewritten by the kernels on every replay."""
    c, h, w = chw
    _set_stages(monkeypatch, True)
    b1, b2 = _make_blocks(c, 1)
    xs = _input(c, h, w).requires_grad_(True)

    def step(b, x):
        y = b(x)
        y.float().square().mean().backward()
        return y

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(b1, xs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    xs.grad = None
    for p in b1.parameters():
        p.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ys = step(b1, xs)

    for it in range(3):
        xn = _input(c, h, w, seed=100 + it)
        with torch.no_grad():
            xs.copy_(xn)
        g.replay()
        torch.cuda.synchronize()
        xe = xn.clone().requires_grad_(True)
        for p in b2.parameters():
            p.grad = None
        ye = step(b2, xe)
        _assert_step_matches(ys, xs, b1, ye, xe, b2)
