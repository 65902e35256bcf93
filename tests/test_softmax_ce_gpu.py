"""GPU tests of the fused softmax-CE kernel (csrc/softmax_ce.hip), its
hipGraph capture, and the engine's mixup step and evaluate() on top of it.

Every test here requires an MI355X."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from edl_amd import ops
    from edl_amd.ops.functional import softmax_cross_entropy
else:
    ops = None

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    # loud check: the HIP extension must be present on a GPU box
    assert ops.available(), "edl_amd._C missing on a GPU box"


def _ref_loss(s32, a, b, lam, eps):
    """fp32 torch reference: the lam-weighted pair of F.cross_entropy."""
    la = F.cross_entropy(s32, a, label_smoothing=eps, reduction="none")
    if b is None:
        return la.mean()
    lb = F.cross_entropy(s32, b, label_smoothing=eps, reduction="none")
    return (lam * la + (1 - lam) * lb).mean()


def _ref_rank(s32, a):
    sa = s32.gather(1, a[:, None])
    col = torch.arange(s32.shape[1], device=s32.device)
    return ((s32 > sa) | ((s32 == sa) & (col < a[:, None]))).sum(1).to(torch.int32)


# the smallest shapes that reach each code path of the kernel
SHAPES = [
    (4, 13),     # scalar only, C < 256
    (7, 1000),   # vector path, B not a power of two
    (3, 1001),   # odd C: unaligned rows must take the scalar path
    (2, 4104),   # > 256*8 elements: several vectors per lane
    (2, 4099),   # the same, scalar
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mixup", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_softmax_ce_forward_backward(dtype, eps, mixup, shape):
    torch.manual_seed(1)
    B, C = shape
    s32 = (torch.randn(B, C, device="cuda") * 4).float()
    a = torch.randint(0, C, (B,), device="cuda")
    b = torch.randint(0, C, (B,), device="cuda") if mixup else None
    lam = torch.rand(B, device="cuda") if mixup else None
    s = s32.to(dtype).requires_grad_(True)

    loss, rank = softmax_cross_entropy(s, a, label_smoothing=eps, labels_b=b,
                                       lam=lam, return_rank=True)
    loss.backward()

    sref = s32.detach().to(dtype).float().requires_grad_(True)
    lref = _ref_loss(sref, a, b, lam, eps)
    lref.backward()

    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert loss.dtype == torch.float32 and s.grad.dtype == dtype
    assert torch.allclose(loss.float(), lref.detach(), atol=tol, rtol=tol), \
        (loss.item(), lref.item())
    assert torch.allclose(s.grad.float(), sref.grad, atol=tol, rtol=tol), \
        (s.grad.float() - sref.grad).abs().max().item()
    assert torch.equal(rank, _ref_rank(sref.detach(), a))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_softmax_ce_lse_output(dtype, shape):
    torch.manual_seed(2)
    B, C = shape
    s = (torch.randn(B, C, device="cuda") * 4).to(dtype)
    a = torch.randint(0, C, (B,), device="cuda")
    loss_row, lse, rank = ops.ext().softmax_ce_forward(s, a, None, None, 0.0)
    ref = torch.logsumexp(s.float(), dim=1)
    assert lse.dtype == torch.float32 and rank.dtype == torch.int32
    assert torch.allclose(lse, ref, atol=1e-5, rtol=1e-5), \
        (lse - ref).abs().max().item()
    assert torch.allclose(
        loss_row, F.cross_entropy(s.float(), a, reduction="none"),
        atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("C", [1000, 1001])
def test_rank_bf16_rows_with_ties(C):
    """bf16 keeps 8 bits of mantissa: 64 rows of C small logits are full
    of exact ties, which must go to the lower index."""
    torch.manual_seed(3)
    B = 64
    s = torch.randn(B, C, device="cuda").to(torch.bfloat16)
    a = torch.randint(0, C, (B,), device="cuda")
    sa = s.gather(1, a[:, None])
    assert int((s == sa).sum()) > B  # the rows do contain ties
    _, rank = softmax_cross_entropy(s, a, return_rank=True)
    assert torch.equal(rank, _ref_rank(s.float(), a))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [13, 1000, 1001])
def test_rank_all_equal_row_and_edge_labels(dtype, C):
    # all-equal logits: rank == label, at index 0, C-1 and in between
    a = torch.tensor([0, C - 1, C // 2, 1], device="cuda")
    s = torch.full((4, C), 0.25, device="cuda", dtype=dtype)
    _, rank = softmax_cross_entropy(s, a, return_rank=True)
    assert torch.equal(rank, a.to(torch.int32))
    # random rows with the label at index 0 and at index C-1
    torch.manual_seed(4)
    s = torch.randn(4, C, device="cuda").to(dtype)
    a = torch.tensor([0, C - 1, 0, C - 1], device="cuda")
    _, rank = softmax_cross_entropy(s, a, return_rank=True)
    assert torch.equal(rank, _ref_rank(s.float(), a))
    # a strict maximum placed there is top-1
    s[torch.arange(4, device="cuda"), a] = 50.0
    _, rank = softmax_cross_entropy(s, a, return_rank=True)
    assert torch.equal(rank, torch.zeros(4, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_out_of_range_labels_are_guarded(dtype):
    """A label outside [0,C) is not dereferenced: it contributes no
    target term to loss or gradient and reports rank = C."""
    torch.manual_seed(5)
    B, C, eps = 4, 1000, 0.1
    s = (torch.randn(B, C, device="cuda") * 4).to(dtype).requires_grad_(True)
    a = torch.tensor([5, -1, C, 1 << 40], device="cuda")
    loss, rank = softmax_cross_entropy(s, a, label_smoothing=eps,
                                       return_rank=True)
    loss.backward()
    sr = s.detach().float().requires_grad_(True)
    rows = torch.logsumexp(sr, 1) - (eps / C) * sr.sum(1)
    ref = (rows.sum() - (1 - eps) * sr[0, 5]) / B
    ref.backward()
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert torch.allclose(loss, ref.detach(), atol=tol, rtol=tol)
    assert torch.allclose(s.grad.float(), sr.grad, atol=tol, rtol=tol)
    assert rank[1:].tolist() == [C, C, C]


def test_softmax_ce_extreme_logits_stable():
    """Large-magnitude logits must not overflow (online max-subtraction)."""
    torch.manual_seed(6)
    B, C = 16, 1000
    for dtype in (torch.float32, torch.bfloat16):
        s = (torch.randn(B, C, device="cuda") * 60).to(dtype).requires_grad_(True)
        a = torch.randint(0, C, (B,), device="cuda")
        b = torch.randint(0, C, (B,), device="cuda")
        loss = softmax_cross_entropy(s, a, label_smoothing=0.1, labels_b=b,
                                     lam=0.4)
        assert torch.isfinite(loss)
        loss.backward()
        assert torch.isfinite(s.grad).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gout_is_honoured(dtype):
    """(3*loss).backward() gives 3x the gradient. The output is rounded
    to the logits' dtype, so compare against the fp32 reference and not
    against 3x the kernel's own result."""
    torch.manual_seed(7)
    B, C = 7, 1000
    s32 = torch.randn(B, C, device="cuda") * 4
    a = torch.randint(0, C, (B,), device="cuda")
    s = s32.to(dtype).requires_grad_(True)
    (3.0 * softmax_cross_entropy(s, a, label_smoothing=0.1)).backward()
    sr = s32.to(dtype).float().requires_grad_(True)
    (3.0 * F.cross_entropy(sr, a, label_smoothing=0.1)).backward()
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert torch.allclose(s.grad.float(), sr.grad, atol=tol, rtol=tol), \
        (s.grad.float() - sr.grad).abs().max().item()
    # 1x the gradient would miss: its peak, ~3*0.9/B, is far above tol
    assert (sr.grad / 3 - sr.grad).abs().max().item() > 10 * tol


def _run_child(tmp_path, name, script, timeout):
    """Run a GPU script in a FRESH process (see
    test_ops_gpu.test_engine_graph_capture_subprocess: capture after
    unrelated GPU activity in the same process can crash the runtime, and
    a crash must not take the suite down). -> the child's RESULT dict."""
    sp = tmp_path / name
    sp.write_text(script)
    env = dict(os.environ)
    env["EDL_REPO"] = REPO
    out = subprocess.run([sys.executable, str(sp)], capture_output=True,
                         text=True, timeout=timeout, cwd=REPO, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert lines, out.stdout + out.stderr
    return json.loads(lines[-1][len("RESULT "):])


CAPTURE_CHILD = r"""
import json, os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.environ["EDL_REPO"])
from edl_amd.ops.functional import softmax_cross_entropy

B, C, eps = 8, 1000, 0.1
torch.manual_seed(0)
dev = "cuda"
logits = (torch.randn(B, C, device=dev) * 4).to(torch.bfloat16).requires_grad_(True)
labels = torch.randint(0, C, (B,), device=dev)
labels_b = torch.randint(0, C, (B,), device=dev)
lam = torch.rand(B, device=dev)

def step():
    loss = softmax_cross_entropy(logits, labels, label_smoothing=eps,
                                 labels_b=labels_b, lam=lam)
    loss.backward()
    return loss

s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    for _ in range(3):
        logits.grad = None
        step()
torch.cuda.current_stream().wait_stream(s)
torch.cuda.synchronize()

logits.grad = None
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    static_loss = step()
static_grad = logits.grad

# new contents in EVERY static buffer, then replay
torch.manual_seed(1)
new_logits = (torch.randn(B, C, device=dev) * 4).to(torch.bfloat16)
with torch.no_grad():
    logits.copy_(new_logits)
labels.copy_(torch.randint(0, C, (B,), device=dev))
labels_b.copy_(torch.randint(0, C, (B,), device=dev))
lam.copy_(torch.rand(B, device=dev))
g.replay()
torch.cuda.synchronize()

sr = new_logits.float().requires_grad_(True)
la = F.cross_entropy(sr, labels, label_smoothing=eps, reduction="none")
lb = F.cross_entropy(sr, labels_b, label_smoothing=eps, reduction="none")
ref = (lam * la + (1 - lam) * lb).mean()
ref.backward()
print("RESULT " + json.dumps({
    "loss": static_loss.item(), "ref": ref.item(),
    "loss_ok": bool(torch.allclose(static_loss.float(), ref.detach(),
                                   atol=2e-2, rtol=2e-2)),
    "grad_err": (static_grad.float() - sr.grad).abs().max().item(),
    "grad_ok": bool(torch.allclose(static_grad.float(), sr.grad,
                                   atol=2e-2, rtol=2e-2)),
    "grad_absmax": sr.grad.abs().max().item(),
}), flush=True)
"""


def test_capture_safety_subprocess(tmp_path):
    """forward+backward captured ONCE on static buffers, every buffer
    overwritten, one replay: the static loss and .grad must be those of
    the NEW contents. Fails if anything syncs during capture or bakes a
    host value (gout, lam, a label) into the graph."""
    res = _run_child(tmp_path, "capture_child.py", CAPTURE_CHILD, timeout=240)
    assert res["loss_ok"], res
    assert res["grad_ok"], res
    # the gradient of a row's two label columns is ~lam/B: far above tol
    # would be vacuous otherwise; check the reference grad is not ~0
    assert res["grad_absmax"] > 0.03, res


def _eval_batches(n, B=8, hw=64, classes=10, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = (torch.randn(B, 3, hw, hw, generator=g) * scale).cuda().contiguous(
            memory_format=torch.channels_last)
        out.append((x, torch.randint(0, classes, (B,), generator=g).cuda()))
    return out


class _FixedLoader:
    def __init__(self, batches):
        self.batches = batches
        self.i = 0

    def next(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        return b


def _small_engine(**kw):
    from edl_amd.train.engine import TrainerEngine

    return TrainerEngine(model="resnet18_vd", per_device_batch=8,
                         num_classes=10, dtype="bf16", base_lr=0.05,
                         use_hip_ops=True, checkpoint_dir=None, **kw).setup()


def test_engine_fused_ce_first_step_matches_default():
    """Same seed, same batch: the first step's loss on the fused kernel
    equals the default F.cross_entropy loss. Both read the same bf16
    logits, so only the forward's run-to-run noise separates them:
    docs/benchmarks.md tabulates 5e-4..8e-4 relative on the loss; the
    bound is 2e-3, about 3x that. track_accuracy leaves the rank on the
    device."""
    x, y = _eval_batches(1, seed=400)[0]
    plain = _small_engine(graph_capture=False)
    fused = _small_engine(graph_capture=False, fused_ce=True,
                          track_accuracy=True)
    assert plain.last_rank is None
    l_plain = plain.train_step(x, y).item()
    l_fused = fused.train_step(x, y).item()
    print("first-step loss: default %.6f fused %.6f" % (l_plain, l_fused))
    assert abs(l_fused - l_plain) <= 2e-3 * abs(l_plain), (l_plain, l_fused)
    r = fused.last_rank
    assert r.is_cuda and r.dtype == torch.int32 and r.shape == (8,)
    assert bool(((r >= 0) & (r < 10)).all())
    assert plain.last_rank is None


def test_engine_eval_freshness():
    """evaluate() after more training must see the CURRENT weights and
    running statistics, not the first eval's cached BN scale/shift or
    repacked conv weights: a warm engine must agree with a cold engine
    that loaded its state_dict.

    Measured on MI355X: see the figures recorded in docs/kernels.md
    ("Eval freshness")."""
    eng = _small_engine(graph_capture=False)
    fixed = _eval_batches(2, seed=100)
    train = _eval_batches(3, seed=200)
    loud = _eval_batches(8, seed=300, scale=8.0)

    eng.model.train()
    for x, y in train:
        eng.train_step(x, y)
    e1 = eng.evaluate(_FixedLoader(fixed), 2)
    assert eng.model.training
    for x, y in loud:  # inputs scaled by 8: the running statistics move far
        eng.train_step(x, y)
    e2 = eng.evaluate(_FixedLoader(fixed), 2)

    cold = _small_engine(graph_capture=False)
    cold.model.load_state_dict(eng.model.state_dict())
    e2_cold = cold.evaluate(_FixedLoader(fixed), 2)
    e2b = eng.evaluate(_FixedLoader(fixed), 2)

    floor = abs(e2["loss"] - e2b["loss"])  # split-K atomic-order noise
    diff = abs(e2["loss"] - e2_cold["loss"])
    bound = max(4 * floor, 2e-3 * abs(e2_cold["loss"]))
    print("eval freshness: e1=%r e2=%r e2_cold=%r e2b=%r floor=%.3e diff=%.3e "
          "bound=%.3e" % (e1, e2, e2_cold, e2b, floor, diff, bound))
    for e in (e1, e2, e2_cold, e2b):
        assert e["samples"] == 16
        assert e["loss"] == e["loss"] and 0.0 <= e["acc1"] <= e["acc5"] <= 1.0
    assert diff <= bound, (e2, e2_cold, floor, bound)


ENGINE_CAPTURE_CHILD = r"""
import json, os, sys
import torch
sys.path.insert(0, os.environ["EDL_REPO"])
from edl_amd.train.engine import TrainerEngine

eng = TrainerEngine(model="resnet18_vd", per_device_batch=8, num_classes=10,
                    dtype="bf16", base_lr=0.05, use_hip_ops=True,
                    checkpoint_dir=None, graph_capture=True, fused_ce=True,
                    track_accuracy=False).setup()
g = torch.Generator().manual_seed(0)
def batch():
    x = torch.randn(8, 3, 64, 64, generator=g).cuda().contiguous(
        memory_format=torch.channels_last)
    return (x, torch.randint(0, 10, (8,), generator=g).cuda(),
            torch.randint(0, 10, (8,), generator=g).cuda())
x, y, yb = batch()
lam = torch.full((8,), 0.7, device="cuda")
ok = eng.maybe_capture(x, y, labels_b=yb, lam=lam)
captured = eng._graph is not None
losses = []
for l in (0.1, 0.5, 0.9):
    x, y, yb = batch()
    loss = eng.replay_step(x, y, labels_b=yb,
                           lam=torch.full((8,), l, device="cuda"))
    torch.cuda.synchronize()
    losses.append(float(loss.item()))
print("RESULT " + json.dumps({"ok": bool(ok), "captured": captured,
                              "losses": losses,
                              "global_step": eng.global_step}), flush=True)
"""


def test_engine_captured_mixup_subprocess(tmp_path):
    """Whole mixup step with the fused loss captured as one hipGraph;
    three replays with different lam tensors."""
    res = _run_child(tmp_path, "engine_capture_child.py", ENGINE_CAPTURE_CHILD,
                     timeout=480)
    assert res["captured"] and res["ok"], res
    assert len(res["losses"]) == 3
    assert all(l == l and abs(l) != float("inf") for l in res["losses"]), res
