"""The classifier head (csrc/head.hip, ops/head.py): global avg-pool + FC,
forward and backward, against fp64 CPU references. Integer operands
(tests/_mfma_exact_common.py) make pooled, logits, dx, dW and db bit-equal
to the reference; two real-valued cases check the rounding under derived
bounds. Measured max(err/bound) on MI355X, (32,2048,7,7,1000) /
(16,512,3,5,10): see docs/kernels.md, head.hip.
"""
import functools

import pytest
import torch

import _mfma_exact_common as X

pytestmark = pytest.mark.gpu

EXACT = [(5, 64, 1, 1, 10, X.ASYM3), (17, 128, 2, 2, 65, X.PM12),
         (33, 512, 4, 4, 63, X.PM1), (32, 2048, 1, 1, 1000, X.PM12),
         (1, 64, 7, 7, 1, X.ASYM3),
         (70, 64, 1, 1, 17, X.PM1)]  # a second 64-row pass
REAL = [(32, 2048, 7, 7, 1000), (16, 512, 3, 5, 10)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _e():
    from edl_amd import ops
    return ops.ext()


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _exact_case(N, C, H, W, K, wvals):
    """CPU operands and fp64 references; the budgets are asserted on the
    references before any kernel output is looked at."""
    gen = torch.Generator().manual_seed(N + 3 * C + 7 * H + 11 * K)
    hw = H * W
    x = (X.ints((N, C, H, W), X.PM1, gen).float() * hw).to(torch.bfloat16)
    w = X.ints((K, C), wvals, gen)
    b = X.ints((K,), X.PM12, gen).float()
    dl = (X.ints((N, K), X.PM12, gen).float() * hw).to(torch.bfloat16)
    pooled = X._d(x).mean((2, 3))
    logits = pooled @ X._d(w).t() + X._d(b)
    dp = X._d(dl) @ X._d(w) / hw
    dw, db = X._d(dl).t() @ pooled, X._d(dl).sum(0)
    for r in (pooled, logits, dp, dw, db):
        assert torch.equal(r, r.round())
    dla, wa = X._d(dl).abs(), X._d(w).abs()
    budget = max(X._d(x).abs().sum((2, 3)).max(),
                 (pooled.abs() @ wa.t() + X._d(b).abs()).max(),
                 (dla @ wa).max(), (dla.t() @ pooled.abs()).max(),
                 dla.sum(0).max()).item()
    assert budget < X.TWO24, budget  # every partial sum, in any order
    for r in (logits, dp):
        assert X.small_share(r) >= 0.9, X.small_share(r)
        if hw == 49:  # 1/49 is inexact in fp32: no tie above 256 may occur
            assert r.abs().max().item() <= 256
    dx = dp[:, :, None, None].expand(N, C, H, W)
    return x, w, b, dl, pooled, logits, dx, dw, db


@pytest.mark.parametrize("N,C,H,W,K,wvals", EXACT)
def test_head_exact(N, C, H, W, K, wvals):
    x, w, b, dl, pooled, logits, dx, dw, db = _exact_case(N, C, H, W, K, wvals)
    e = _e()
    got_l, got_p = e.head_fwd(_cl(x), w.cuda(), b.cuda())
    X.check_exact(got_p, pooled, "pooled")
    X.check_exact(got_l, logits, "logits")
    nob = e.head_fwd(_cl(x), w.cuda())[0]
    X.check_exact(nob, logits - X._d(b), "logits without bias")
    got_dx, got_dw, got_db = e.head_bwd(dl.cuda(), got_p, w.cuda(), H, W, True)
    assert got_dx.is_contiguous(memory_format=torch.channels_last)
    X.check_exact(got_dx, dx, "dx")
    X.check_exact(got_dw, dw, "dW")
    X.check_exact(got_db, db, "db")
    # direct-grad mode: add into integer-filled targets, return nothing
    gen = torch.Generator().manual_seed(1)
    pw = X.ints((K, C), X.PM12, gen).float()
    pb = X.ints((K,), X.ASYM3, gen).float()
    tw, tb = pw.cuda(), pb.cuda()
    out = e.head_bwd(dl.cuda(), got_p, w.cuda(), H, W, False, tw, tb)
    assert out == (None, None, None)
    X.check_exact(tw, X._d(pw) + dw, "dw_out")
    X.check_exact(tb, X._d(pb) + db, "db_out")


@pytest.mark.parametrize("N,C,H,W,K", REAL)
def test_head_real_bounds(N, C, H, W, K):
    gen = torch.Generator().manual_seed(N + K)
    hw = H * W
    x = torch.randn((N, C, H, W), generator=gen).to(torch.bfloat16)
    w = (torch.randn((K, C), generator=gen) * C ** -0.5).to(torch.bfloat16)
    b = torch.randn((K,), generator=gen)
    dl = torch.randn((N, K), generator=gen).to(torch.bfloat16)
    e = _e()
    lg, p = e.head_fwd(_cl(x), w.cuda(), b.cuda())
    dx, dw, db = e.head_bwd(dl.cuda(), p, w.cuda(), H, W, True)
    xd, wd, dld, pd = X._d(x), X._d(w), X._d(dl), X._d(p)
    ratio = {}
    pref = xd.mean((2, 3))
    pbound = 2.0 ** -8 * pref.abs() + 2 * hw * 2.0 ** -24 * xd.abs().mean((2, 3))
    ratio["pooled"] = ((pd - pref).abs() / pbound).max().item()
    ratio["logits"] = X.bound_ratio(
        lg, pd @ wd.t() + X._d(b), pd.abs() @ wd.abs().t() + X._d(b).abs(),
        C + 1)
    dref = (dld @ wd / hw)[:, :, None, None].expand(N, C, H, W)
    E = (X.accum_bound(dld.abs() @ wd.abs(), K) / hw)[:, :, None, None]
    ratio["dx"] = ((X._d(dx) - dref).abs()
                   / (2.0 ** -8 * (dref.abs() + E) + E)).max().item()
    ratio["dW"] = X.bound_ratio(dw, dld.t() @ pd, dld.abs().t() @ pd.abs(), N)
    ratio["db"] = X.bound_ratio(db, dld.sum(0), dld.abs().sum(0), N)
    print("head max(err/bound)", (N, C, H, W, K), ratio)
    assert all(v <= 1.0 for v in ratio.values()), ratio


def _refusal(name):
    bf = dict(dtype=torch.bfloat16, device="cuda")
    x = _cl(torch.ones(2, 64, 2, 2, dtype=torch.bfloat16))
    w, dl, p = torch.ones(8, 64, **bf), torch.ones(2, 8, **bf), \
        torch.ones(2, 64, **bf)
    e = _e()
    if name == "dtype":
        return lambda: e.head_fwd(x.half(), w)
    if name == "c_mod_64":
        return lambda: e.head_fwd(_cl(torch.ones(2, 96, 1, 1).bfloat16()),
                                  torch.ones(8, 96, **bf))
    if name == "rows":
        return lambda: e.head_fwd(_cl(torch.ones(513, 64, 1, 1).bfloat16()), w)
    if name == "misaligned":
        return lambda: e.head_fwd(x, torch.ones(8 * 64 + 1, **bf)[1:].view(8, 64))
    if name == "strided":
        return lambda: e.head_fwd(x, torch.ones(8, 128, **bf)[:, ::2])
    if name == "dw_shape":
        return lambda: e.head_bwd(dl, p, w, 2, 2, False,
                                  torch.zeros(64, 8, device="cuda"))
    if name == "dw_dtype":
        return lambda: e.head_bwd(dl, p, w, 2, 2, False,
                                  torch.zeros(8, 64, **bf))


@pytest.mark.parametrize("name", ["dtype", "c_mod_64", "rows", "misaligned",
                                  "strided", "dw_shape", "dw_dtype"])
def test_head_binding_refuses(name):
    with pytest.raises(RuntimeError, match="head_"):
        _refusal(name)()


@pytest.mark.parametrize("on", [1, 0])
def test_head_route(monkeypatch, on):
    from edl_amd.models.resnet_vd import resnet18_vd
    from edl_amd.ops import head
    e, calls = _e(), {}

    def counted(name, fn):
        def f(*a):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a)
        return f

    for name in ("head_fwd", "head_bwd"):
        monkeypatch.setattr(e, name, counted(name, getattr(e, name)))
    monkeypatch.setattr(head, "_HEAD", bool(on))
    torch.manual_seed(0)
    m = resnet18_vd(num_classes=10).cuda().to(memory_format=torch.channels_last)
    x = _cl(torch.randn(2, 3, 64, 64))
    feats = []
    m.stages.register_forward_hook(lambda mod, i, o: feats.append(o))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
        today = m.fc(m.avgpool(feats[0]).flatten(1))
    y.float().sum().backward()
    assert y.shape == (2, 10) and y.dtype == torch.bfloat16
    assert m.fc.weight.grad is not None and m.fc.bias.grad is not None
    assert all(p.grad is not None for p in m.stem.parameters())
    if on:
        assert calls == {"head_fwd": 1, "head_bwd": 1}, calls
    else:
        assert calls == {}
        assert torch.equal(y, today)
