"""The residual-gradient add folded into the 1x1 dgrad GEMM (GPU).

A bottleneck block's input feeds conv0 and the shortcut. conv0 (a 1x1
Conv2dFast) can fork its input: the shortcut consumes the pass-through, both
gradients arrive in conv0's backward, and gemm_bt_add sums them in the GEMM
epilogue in place of autograd's elementwise add. Anything that does not fit
(an unused fork, a non-dense gradient, the switch off) takes the old route.

Blocks: batch 2 at 9x11 (M = 198: one ragged tile); identity, stride-2 and
first-of-stage-1, i.e. the shortcut gradient coming from bn_bwd's dres, from
AvgPool2x2's backward and from the projection conv's dgrad."""
import copy

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu

N, H, W = 2, 9, 11
BLOCKS = [(256, 64, 1, False), (256, 128, 2, False), (64, 64, 1, True)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ext():
    from edl_amd import ops

    return ops.ext()


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


class _AtenAdds(TorchDispatchMode):
    """Counts torch's own add kernels (autograd's gradient sums included)."""

    def __init__(self):
        super().__init__()
        self.count = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.overloadpacket in (torch.ops.aten.add, torch.ops.aten.add_):
            self.count += 1
        return func(*args, **(kwargs or {}))


def _set_switch(monkeypatch, on):
    import edl_amd.ops.conv as conv_mod

    monkeypatch.setattr(conv_mod, "_DGRAD_ADD", on)


def _cl(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(*shape, device="cuda", generator=g).to(torch.bfloat16)
    return t.contiguous(memory_format=torch.channels_last)


def _rows(t4):
    return t4.permute(0, 2, 3, 1).reshape(-1, t4.shape[1])


def _conv1x1(cin, cout):
    from edl_amd.ops.conv import Conv2dFast

    torch.manual_seed(5)
    return Conv2dFast(cin, cout, 1, bias=False).cuda().to(torch.bfloat16)


def _wt(conv):
    co, ci = conv.out_channels, conv.in_channels
    return conv.weight.detach().view(co, ci).t().contiguous()


@pytest.mark.parametrize("cin,cout", [(256, 64), (64, 64)])
def test_fork_sums_in_the_gemm_epilogue(cin, cout, monkeypatch):
    """x.grad is bit-equal to gemm_bt(gy, wt) + gr (no split-K, no atomics
    on this path), computed by ONE gemm_bt_add and no torch add."""
    e = _ext()
    _set_switch(monkeypatch, True)
    conv = _conv1x1(cin, cout)
    x = _cl((N, cin, H, W), 1).requires_grad_(True)
    gy = _cl((N, cout, H, W), 2)
    gr = _cl((N, cin, H, W), 3)
    want = e.gemm_bt(_rows(gy), _wt(conv)) + _rows(gr)
    gy0, gr0 = gy.clone(), gr.clone()

    spy = _Spy(monkeypatch, ["gemm_bt", "gemm_bt_add"])
    y, x_fork = conv(x, fork=True)
    assert x_fork is not x and x_fork.data_ptr() == x.data_ptr()
    assert torch.equal(x_fork, x)
    loss = (y * gy).sum() + (x_fork * gr).sum()
    spy.reset()
    adds = _AtenAdds()
    with adds:
        loss.backward()
    assert spy.calls == {"gemm_bt": 0, "gemm_bt_add": 1}
    assert adds.count == 0
    assert torch.equal(_rows(x.grad), want)
    assert torch.equal(gy, gy0) and torch.equal(gr, gr0)


def test_unused_fork_is_the_plain_dgrad(monkeypatch):
    e = _ext()
    _set_switch(monkeypatch, True)
    conv = _conv1x1(256, 64)
    x = _cl((N, 256, H, W), 1).requires_grad_(True)
    gy = _cl((N, 64, H, W), 2)
    want = e.gemm_bt(_rows(gy), _wt(conv))
    spy = _Spy(monkeypatch, ["gemm_bt", "gemm_bt_add"])
    y, _ = conv(x, fork=True)
    spy.reset()
    (y * gy).sum().backward()
    assert spy.calls == {"gemm_bt": 1, "gemm_bt_add": 0}
    assert torch.equal(_rows(x.grad), want)


def test_only_the_fork_used(monkeypatch):
    _set_switch(monkeypatch, True)
    conv = _conv1x1(256, 64)
    x = _cl((N, 256, H, W), 1).requires_grad_(True)
    gr = _cl((N, 256, H, W), 3)
    _, x_fork = conv(x, fork=True)
    (x_fork * gr).sum().backward()
    assert torch.equal(x.grad, gr)
    assert conv.weight.grad is None


def test_non_dense_fork_gradient_falls_back(monkeypatch):
    """sum()'s backward hands over an expanded (stride-0) gradient: torch
    adds it after the plain GEMM, and the result is the same."""
    e = _ext()
    _set_switch(monkeypatch, True)
    conv = _conv1x1(256, 64)
    x = _cl((N, 256, H, W), 1).requires_grad_(True)
    gy = _cl((N, 64, H, W), 2)
    want = e.gemm_bt(_rows(gy), _wt(conv)) + 1
    spy = _Spy(monkeypatch, ["gemm_bt", "gemm_bt_add"])
    y, x_fork = conv(x, fork=True)
    spy.reset()
    ((y * gy).sum() + x_fork.sum()).backward()
    assert spy.calls == {"gemm_bt": 1, "gemm_bt_add": 0}
    assert torch.equal(_rows(x.grad), want)


def test_switch_off_and_no_grad_return_the_input(monkeypatch):
    conv = _conv1x1(256, 64)
    x = _cl((N, 256, H, W), 1).requires_grad_(True)
    _set_switch(monkeypatch, False)
    y, x_fork = conv(x, fork=True)
    assert x_fork is x
    _set_switch(monkeypatch, True)
    with torch.no_grad():
        y2, x_fork = conv(x, fork=True)
    assert x_fork is x and torch.equal(y, y2)
    xd = x.detach()  # nothing to sum for an input without a gradient
    y3, x_fork = conv(xd, fork=True)
    assert x_fork is xd and torch.equal(y, y3)


# ---- BottleneckVd ----


def _make_blocks(cin, planes, stride, if_first):
    import edl_amd.ops.conv as conv_mod
    from edl_amd.models.resnet_vd import BottleneckVd

    torch.manual_seed(32)
    b1 = BottleneckVd(cin, planes, stride=stride,
                      if_first=if_first).cuda().train()
    for mod in b1.modules():
        if isinstance(mod, conv_mod.Conv2dFast):
            mod.to(torch.bfloat16)
    return b1, copy.deepcopy(b1)


def _assert_step_matches(y1, x1, b1, y2, x2, b2):
    assert torch.allclose(y1.float(), y2.float(), atol=1e-2, rtol=1e-2)
    assert torch.allclose(x1.grad.float(), x2.grad.float(), atol=1e-2,
                          rtol=1e-2)
    for p1, p2 in zip(b1.parameters(), b2.parameters()):
        assert (p1.grad is None) == (p2.grad is None)
        if p1.grad is not None:
            assert torch.allclose(p1.grad.float(), p2.grad.float(),
                                  atol=5e-2, rtol=5e-2), p1.shape


def _step(b, x):
    y = b(x)
    y.float().square().mean().backward()
    return y


@pytest.mark.parametrize("cfg", BLOCKS)
def test_bottleneck_step_fused_vs_switch_off(cfg, monkeypatch):
    cin = cfg[0]
    b1, b2 = _make_blocks(*cfg)
    x1 = _cl((N, cin, H, W), 33).requires_grad_(True)
    x2 = x1.detach().clone().requires_grad_(True)
    spy = _Spy(monkeypatch, ["gemm_bt_add"])

    _set_switch(monkeypatch, True)
    y1 = _step(b1, x1)
    assert spy.calls["gemm_bt_add"] == 1

    spy.reset()
    _set_switch(monkeypatch, False)
    y2 = _step(b2, x2)
    assert spy.calls["gemm_bt_add"] == 0

    _assert_step_matches(y1, x1, b1, y2, x2, b2)


def test_graph_capture_replay(monkeypatch):
    """Forward+backward of the identity block captured and replayed three
    times with new input, against eager runs with the switch off."""
    cfg = BLOCKS[0]
    cin = cfg[0]
    _set_switch(monkeypatch, True)
    b1, b2 = _make_blocks(*cfg)
    xs = _cl((N, cin, H, W), 33).requires_grad_(True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _step(b1, xs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    xs.grad = None
    for p in b1.parameters():
        p.grad = None
    spy = _Spy(monkeypatch, ["gemm_bt_add"])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ys = _step(b1, xs)
    assert spy.calls["gemm_bt_add"] == 1

    _set_switch(monkeypatch, False)
    for it in range(3):
        xn = _cl((N, cin, H, W), 100 + it)
        with torch.no_grad():
            xs.copy_(xn)
        g.replay()
        torch.cuda.synchronize()
        xe = xn.clone().requires_grad_(True)
        for p in b2.parameters():
            p.grad = None
        ye = _step(b2, xe)
        _assert_step_matches(ys, xs, b1, ye, xe, b2)
