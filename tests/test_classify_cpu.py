"""Classification loss / accuracy / mixup / eval on CPU: the torch
reference path of softmax_cross_entropy (same formulas and tie rule as
csrc/softmax_ce.hip), MixupLoader, the engine's mixup step and
evaluate(), and the trainer's new flags."""
import pytest
import torch
import torch.nn.functional as F

from edl_amd.data.mixup import MixupLoader
from edl_amd.ops.functional import softmax_cross_entropy
from edl_amd.train.engine import TrainerEngine


def _rank_def(s, a):
    """rank_i = #{j: s_ij > s_ia} + #{j < a_i: s_ij == s_ia}, by loops."""
    out = []
    for i in range(s.shape[0]):
        sa = s[i, a[i]]
        out.append(sum(1 for j in range(s.shape[1])
                       if s[i, j] > sa or (s[i, j] == sa and j < a[i])))
    return torch.tensor(out, dtype=torch.int32)


@pytest.mark.parametrize("shape", [(4, 13), (7, 1000)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_reference_loss_and_grad(shape, eps):
    torch.manual_seed(0)
    B, C = shape
    s = (torch.randn(B, C) * 3).requires_grad_(True)
    a = torch.randint(0, C, (B,))
    loss = softmax_cross_entropy(s, a, label_smoothing=eps)
    loss.backward()
    sr = s.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(sr, a, label_smoothing=eps)
    ref.backward()
    # fp32 on both sides: a few ulp of a loss of size ~10
    assert torch.allclose(loss, ref.detach(), atol=1e-5, rtol=1e-6), \
        (loss.item(), ref.item())
    assert torch.allclose(s.grad, sr.grad, atol=1e-6), \
        (s.grad - sr.grad).abs().max().item()


@pytest.mark.parametrize("shape", [(4, 13), (7, 1000)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam_kind", ["float", "tensor"])
def test_reference_mixup_loss_and_grad(shape, eps, lam_kind):
    torch.manual_seed(1)
    B, C = shape
    s = (torch.randn(B, C) * 3).requires_grad_(True)
    a = torch.randint(0, C, (B,))
    b = torch.randint(0, C, (B,))
    lam_t = torch.full((B,), 0.3) if lam_kind == "float" else torch.rand(B)
    lam = 0.3 if lam_kind == "float" else lam_t
    loss = softmax_cross_entropy(s, a, label_smoothing=eps, labels_b=b, lam=lam)
    loss.backward()
    sr = s.detach().clone().requires_grad_(True)
    ref = (lam_t * F.cross_entropy(sr, a, label_smoothing=eps, reduction="none")
           + (1 - lam_t) * F.cross_entropy(sr, b, label_smoothing=eps,
                                           reduction="none")).mean()
    ref.backward()
    assert torch.allclose(loss, ref.detach(), atol=1e-5, rtol=1e-6), \
        (loss.item(), ref.item())
    assert torch.allclose(s.grad, sr.grad, atol=1e-6), \
        (s.grad - sr.grad).abs().max().item()


def test_labels_b_and_lam_go_together():
    s = torch.randn(2, 5)
    y = torch.tensor([0, 1])
    with pytest.raises(ValueError):
        softmax_cross_entropy(s, y, labels_b=y)
    with pytest.raises(ValueError):
        softmax_cross_entropy(s, y, lam=0.5)


def test_rank_matches_topk_on_random_rows():
    torch.manual_seed(2)
    B, C = 64, 50
    s = torch.randn(B, C)
    a = torch.randint(0, C, (B,))
    loss, rank = softmax_cross_entropy(s, a, return_rank=True)
    assert rank.dtype == torch.int32 and rank.shape == (B,)
    assert torch.equal(rank, _rank_def(s, a))
    in_top5 = (s.topk(5, dim=1).indices == a[:, None]).any(1)
    assert torch.equal(rank < 5, in_top5)
    in_top1 = s.argmax(1) == a
    assert torch.equal(rank < 1, in_top1)
    assert torch.allclose(loss, F.cross_entropy(s, a), atol=1e-5)


def test_rank_ties_go_to_the_lower_index():
    C = 9
    s = torch.full((C, C), 0.5)
    a = torch.arange(C)
    _, rank = softmax_cross_entropy(s, a, return_rank=True)
    assert torch.equal(rank, a.to(torch.int32))


def test_rank_three_classes_always_top5():
    torch.manual_seed(3)
    s = torch.randn(32, 3)
    a = torch.randint(0, 3, (32,))
    _, rank = softmax_cross_entropy(s, a, return_rank=True)
    assert bool((rank < 5).all())


def test_out_of_range_label_has_no_target_term():
    torch.manual_seed(4)
    C = 7
    s = torch.randn(2, C, requires_grad=True)
    y = torch.tensor([3, C])
    loss, rank = softmax_cross_entropy(s, y, label_smoothing=0.1,
                                       return_rank=True)
    sd = s.detach()
    row1 = torch.logsumexp(sd[1], 0) - 0.1 / C * sd[1].sum()
    row0 = F.cross_entropy(sd[:1], y[:1], label_smoothing=0.1)
    assert torch.allclose(loss, (row0 + row1) / 2, atol=1e-6)
    assert rank[1].item() == C


class _FixedLoader:
    def __init__(self, batches):
        self.batches = batches
        self.i = 0

    def next(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        return b


def _image_batches(n, B=8, classes=10, hw=8, channels_last=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.randn(B, 3, hw, hw, generator=g)
        if channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        out.append((x, torch.randint(0, classes, (B,), generator=g)))
    return out


def test_mixup_loader_batch():
    batches = _image_batches(3, channels_last=True)
    m1 = MixupLoader(_FixedLoader(batches), alpha=0.2, seed=11)
    m2 = MixupLoader(_FixedLoader(batches), alpha=0.2, seed=11)
    m3 = MixupLoader(_FixedLoader(batches), alpha=0.2, seed=12)
    differs = False
    for x, y in batches:
        xm, ya, yb, lam = m1.next()
        xm2, ya2, yb2, lam2 = m2.next()
        _, _, yb3, lam3 = m3.next()
        # deterministic per seed
        assert torch.equal(xm, xm2) and torch.equal(yb, yb2)
        assert torch.equal(lam, lam2)
        differs |= not torch.equal(lam, lam3) or not torch.equal(yb, yb3)
        assert torch.equal(ya, y)
        assert torch.equal(yb.sort().values, y.sort().values)
        assert lam.shape == (x.shape[0],) and lam.dtype == torch.float32
        assert bool((lam == lam[0]).all())  # one draw per batch
        assert 0.0 <= lam[0].item() <= 1.0
        assert xm.is_contiguous(memory_format=torch.channels_last)
        # x_mixed = lam*x + (1-lam)*x[perm]: recover perm from the labels'
        # partner rows by checking the blend against every candidate
        l = lam[0].item()
        for i in range(x.shape[0]):
            resid = (xm[i] - l * x[i]) / max(1 - l, 1e-12)
            if 1 - l > 1e-3:
                j = int(((x - resid) ** 2).flatten(1).sum(1).argmin())
                assert y[j] == yb[i]
    assert differs  # another seed draws another sequence


def test_mixup_alpha_is_honoured():
    """Beta(a,a) has mean 1/2 and variance 1/(4(2a+1)): 0.179 at a=0.2
    (mass at the ends) and 0.0147 at a=8 (mass in the middle). Over 200
    draws the sample mean has sd <= 0.03, so +-0.15 is a 5-sigma bound;
    the sample variance has sd ~0.007 at a=0.2, so the thresholds 0.12
    and 0.04 sit many sigma from both true values."""
    batches = _image_batches(1, B=2)
    for alpha, check in ((0.2, lambda v: v > 0.12), (8.0, lambda v: v < 0.04)):
        m = MixupLoader(_FixedLoader(batches), alpha=alpha, seed=5)
        lams = torch.tensor([m.next()[3][0].item() for _ in range(200)])
        assert bool(((lams >= 0) & (lams <= 1)).all())
        assert abs(lams.mean().item() - 0.5) < 0.15, lams.mean().item()
        assert check(lams.var().item()), (alpha, lams.var().item())


def _cpu_engine(**kw):
    return TrainerEngine(model="resnet18_vd", per_device_batch=2, dtype="fp32",
                         channels_last=False, use_hip_ops=False,
                         graph_capture=False, num_classes=4, **kw).setup()


def test_engine_mixup_step_and_lam_one_equals_plain():
    torch.manual_seed(0)
    x = torch.randn(2, 3, 32, 32)
    y = torch.tensor([1, 3])
    yb = torch.tensor([0, 2])
    plain = _cpu_engine()
    mixed = _cpu_engine()     # same seed in setup(): identical weights
    l_plain = plain.train_step(x, y)
    l_one = mixed.train_step(x, y, labels_b=yb, lam=torch.ones(2))
    assert torch.allclose(l_plain, l_one, atol=1e-5), (l_plain, l_one)
    # a genuine mix runs and gives a finite, different loss
    l_half = mixed.train_step(x, y, labels_b=yb, lam=torch.full((2,), 0.5))
    assert torch.isfinite(l_half)
    # replay_step passes the mixup labels through when nothing is captured
    l_rep = mixed.replay_step(x, y, labels_b=yb, lam=torch.full((2,), 0.5))
    assert torch.isfinite(l_rep)


def test_engine_track_accuracy_keeps_rank():
    torch.manual_seed(0)
    eng = _cpu_engine(track_accuracy=True)
    assert eng.last_rank is None
    x = torch.randn(2, 3, 32, 32)
    y = torch.tensor([1, 3])
    eng.train_step(x, y)
    assert eng.last_rank.shape == (2,)
    assert bool(((eng.last_rank >= 0) & (eng.last_rank < 4)).all())


def test_engine_default_loss_is_unchanged():
    eng = _cpu_engine()
    assert eng.fused_ce is False and eng.track_accuracy is False
    torch.manual_seed(6)
    logits = torch.randn(5, 4)
    labels = torch.randint(0, 4, (5,))
    want = F.cross_entropy(logits.float(), labels, label_smoothing=0.1)
    assert torch.equal(eng._loss(logits, labels), want)
    # and the fused flag computes the same quantity another way
    fused = _cpu_engine(fused_ce=True)
    assert torch.allclose(fused._loss(logits, labels), want, atol=1e-6)


def test_engine_evaluate():
    eng = _cpu_engine()
    batches = _image_batches(3, B=2, classes=4, hw=32, seed=7)
    eng.model.train()
    res = eng.evaluate(_FixedLoader(batches), steps=3)
    assert set(res) == {"loss", "acc1", "acc5", "samples"}
    assert res["samples"] == 3 * 2
    assert 0.0 <= res["acc1"] <= res["acc5"] <= 1.0
    assert res["acc5"] == 1.0          # 4 classes: every row is top-5
    assert res["loss"] > 0
    assert eng.model.training          # mode restored
    eng.model.eval()
    eng.evaluate(_FixedLoader(batches), steps=1)
    assert not eng.model.training
    # no gradient state and no step were produced
    assert eng.global_step == 0


EVAL_WORKER = r"""
import json, os, sys
import torch
sys.path.insert(0, os.environ["EDL_REPO"])
from edl_amd.train import dist as edist
from edl_amd.train.engine import TrainerEngine

class Loader:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
    def next(self):
        return (torch.randn(2, 3, 32, 32, generator=self.g),
                torch.randint(0, 4, (2,), generator=self.g))

eng = TrainerEngine(model="resnet18_vd", per_device_batch=2, dtype="fp32",
                    channels_last=False, use_hip_ops=False,
                    graph_capture=False, num_classes=4).setup()
res = eng.evaluate(Loader(70 + eng.env.global_rank), 2)
print("RESULT " + json.dumps(res), flush=True)
edist.barrier(eng.device)
edist.cleanup()
"""


def test_engine_evaluate_world2_sums_over_ranks(tmp_path):
    """Two gloo ranks evaluate different batches; ONE all_reduce makes
    both report the result of a single process that saw all of them."""
    import json
    import os
    import subprocess
    import sys

    from edl_amd.utils.net import find_free_port

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp = tmp_path / "eval_worker.py"
    sp.write_text(EVAL_WORKER)
    port = find_free_port()
    port = port[0] if isinstance(port, list) else port
    procs = []
    for rank in range(2):
        env = dict(os.environ)
        env.update({"EDL_REPO": repo, "CUDA_VISIBLE_DEVICES": "",
                    "RANK": str(rank), "LOCAL_RANK": str(rank),
                    "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port)})
        env.pop("EDL_CHECKPOINT_DIR", None)
        procs.append(subprocess.Popen(
            [sys.executable, str(sp)], env=env, cwd=str(tmp_path),
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    got = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=170)
            assert p.returncode == 0, out
            line = [l for l in out.splitlines() if l.startswith("RESULT ")][-1]
            got.append(json.loads(line[len("RESULT "):]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert got[0] == got[1]
    assert got[0]["samples"] == 2 * 2 * 2

    class Both:
        def __init__(self):
            self.gens = [torch.Generator().manual_seed(70 + r) for r in (0, 1)]
            self.i = 0

        def next(self):
            g = self.gens[self.i // 2]
            self.i += 1
            return (torch.randn(2, 3, 32, 32, generator=g),
                    torch.randint(0, 4, (2,), generator=g))

    # rank 0 broadcasts its weights (seed 42): the single engine's weights
    ref = _cpu_engine().evaluate(Both(), 4)
    assert ref["samples"] == 8
    assert got[0]["loss"] == pytest.approx(ref["loss"], abs=1e-5)
    assert got[0]["acc1"] == pytest.approx(ref["acc1"], abs=1e-9)
    assert got[0]["acc5"] == pytest.approx(ref["acc5"], abs=1e-9)


def test_cli_defaults():
    from edl_amd.train.train_resnet import parse_args

    a = parse_args([])
    assert a.label_smoothing == 0.1
    assert a.use_mixup == 0
    assert a.mixup_alpha == 0.2
    assert a.fused_ce == 0
    assert a.eval_steps == 0
