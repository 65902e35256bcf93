"""Global-norm gradient clipping on CPU buckets (the torch path of
ops/clip.py and of the optimizers' clip_state): numerics against
torch.nn.utils.clip_grad_norm_ + torch.optim under the tolerance rule of
_adam_common, the non-finite skip, a 2-rank gloo run, and the engine /
CLI / strategy plumbing."""
import math
import os
import subprocess
import sys

import pytest
import torch

import _adam_common as C
import _clip_common as CC
from edl_amd.ops.clip import GradClipper
from edl_amd.train.engine import TrainerEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["sgd", "adam", "adamw"]


def _fused_run(kind, grads, max_norm, skip_nonfinite=False):
    m, _ = CC.model()
    _, opt, clipper = CC.make_fused(m, kind, max_norm, skip_nonfinite)
    out, states = [], []
    for g in grads:
        st = CC.fused_step(m, opt, clipper, g)
        states.append(st.clone())
        out.append(CC.fused_state(m, opt, kind))
    return out, states, opt, clipper


@pytest.mark.parametrize("kind", KINDS)
def test_matches_clip_grad_norm_over_six_steps(kind):
    _, grads = CC.model()
    max_norm = CC.max_norm_for(grads)
    clipped = CC.clipped_steps(grads, max_norm)
    assert any(clipped) and not all(clipped), clipped  # straddles the bound
    truth = CC.torch_run(kind, torch.float64, grads, max_norm)
    ref = C.run_errors(CC.torch_run(kind, torch.float32, grads, max_norm),
                       truth)
    got, states, _, clipper = _fused_run(kind, grads, max_norm)
    C.check(C.run_errors(got, truth), ref, "cpu clip " + kind)
    for g, st, was_clipped in zip(grads, states, clipped):
        norm = float((g * C.GRAD_SCALE).norm())
        assert abs(float(st[1]) - norm) <= 2.0 ** -23 * norm
        assert (float(st[0]) < 1.0) == was_clipped
        assert float(st[2]) == 0.0 and float(st[3]) == 0.0
    assert clipper.norm.data_ptr() == clipper.state[1:].data_ptr()


def test_norm_only_mode_is_bitwise_the_unclipped_step():
    """max_norm=None: coef == 1, and the step equals one without a clip
    state bit for bit."""
    for kind in KINDS:
        _, grads = CC.model()
        got, states, _, _ = _fused_run(kind, grads, None)
        m, _ = CC.model()
        _, opt, _ = CC.make_fused(m, kind, None)
        for g in grads:
            CC.set_grads(m, g)
            opt.step()
        for a, b in zip(got[-1], CC.fused_state(m, opt, kind)):
            assert torch.equal(a, b)
        assert all(float(s[0]) == 1.0 and float(s[1]) > 0 for s in states)


@pytest.mark.parametrize("kind", KINDS)
def test_skip_nonfinite_leaves_the_step_out(kind):
    """A NaN planted in step 3: p, m, v and the step counter keep their
    bits, nskipped counts it, and the run equals a torch run that never
    saw step 3."""
    _, grads = CC.model()
    max_norm = CC.max_norm_for(grads)
    bad = [g.clone() for g in grads]
    bad[2][123] = float("nan")
    m, _ = CC.model()
    _, opt, clipper = CC.make_fused(m, kind, max_norm, skip_nonfinite=True)
    got = []
    for t, g in enumerate(bad):
        before = CC.fused_state(m, opt, kind)
        count = getattr(opt, "step_count", None)
        st = CC.fused_step(m, opt, clipper, g)
        after = CC.fused_state(m, opt, kind)
        if t == 2:
            assert float(st[2]) == 1.0 and float(st[0]) == 0.0
            assert math.isnan(float(st[1]))
            for a, b in zip(before, after):
                assert torch.equal(a, b)
            assert getattr(opt, "step_count", None) == count
        else:
            assert float(st[2]) == 0.0
            got.append(after)
    assert float(clipper.skipped) == 1.0
    if kind != "sgd":
        assert opt.step_count == C.STEPS - 1
    truth = CC.torch_run(kind, torch.float64, grads, max_norm, skip_steps=(2,))
    ref = C.run_errors(
        CC.torch_run(kind, torch.float32, grads, max_norm, skip_steps=(2,)),
        truth)
    C.check(C.run_errors(got, truth), ref, "cpu skip " + kind)


@pytest.mark.parametrize("kind", KINDS)
def test_nan_without_skip_propagates_as_torch(kind):
    _, grads = CC.model()
    max_norm = CC.max_norm_for(grads)
    bad = [g.clone() for g in grads[:3]]
    bad[2][123] = float("nan")
    want = CC.torch_run(kind, torch.float32, bad, max_norm)[-1]
    got, states, _, clipper = _fused_run(kind, bad, max_norm)
    for a, b in zip(got[-1], want):
        assert bool(torch.isnan(b).all())  # torch: everything is NaN
        assert bool(torch.isnan(a).all())
    assert math.isnan(float(states[-1][0])) and float(states[-1][2]) == 0.0
    assert float(clipper.skipped) == 0.0


def test_inf_norm_without_skip_gives_coef_zero():
    """torch's formula on an inf norm: max_norm / inf = 0."""
    m, grads = CC.model()
    _, opt, clipper = CC.make_fused(m, "sgd", 1.0)
    g = grads[0].clone()
    g[5] = float("inf")
    CC.set_grads(m, g)
    st = clipper.run(C.GRAD_SCALE)
    assert float(st[0]) == 0.0 and math.isinf(float(st[1]))


def test_rebuild_rematerialises_and_keeps_the_count():
    _, grads = CC.model()
    max_norm = CC.max_norm_for(grads)
    ma, _ = CC.model()
    mb, _ = CC.model()
    _, oa, ca = CC.make_fused(ma, "adamw", max_norm, skip_nonfinite=True)
    rb, ob, cb = CC.make_fused(mb, "adamw", max_norm, skip_nonfinite=True)
    bad = grads[0].clone()
    bad[0] = float("inf")
    for g in [grads[0], bad, grads[1]]:
        CC.fused_step(ma, oa, ca, g)
        CC.fused_step(mb, ob, cb, g)
    rb.rebuild(0.001)  # one bucket becomes three
    assert len(rb._buckets) == 3
    for g in grads[2:5]:
        sa = CC.fused_step(ma, oa, ca, g)
        sb = CC.fused_step(mb, ob, cb, g)
        assert abs(float(sa[1]) - float(sb[1])) <= 2.0 ** -23 * float(sa[1])
    # the clipper reads the NEW flats (the old ones no longer get gradients)
    assert [b.data_ptr() for b in cb._bufs] == [
        b.buffer.data_ptr() for b in rb._buckets]
    assert float(cb.skipped) == float(ca.skipped) == 1.0
    assert ob.step_count == oa.step_count == 5


def _engine(**kw):
    return TrainerEngine(
        model="mnist_mlp", per_device_batch=8, num_classes=10, base_lr=1e-2,
        momentum=0.0, weight_decay=0.0, label_smoothing=0.0, dtype="fp32",
        channels_last=False, use_hip_ops=False, **kw)


def test_engine_clips_the_update():
    """momentum 0, decay 0: ||dp|| = lr * min(norm, max_norm)."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(8, 1, 28, 28, generator=gen)
    y = torch.randint(0, 10, (8,), generator=gen)
    probe = _engine(skip_nonfinite=True).setup()  # norm-only + skip
    assert probe.clipper is not None and probe.clipper.max_norm == math.inf
    probe.train_step(x, y)
    norm = float(probe.last_grad_norm)
    assert norm > 0 and float(probe.skipped_steps) == 0.0
    for max_norm in (norm / 8, norm * 8):
        eng = _engine(clip_grad_norm=max_norm).setup()
        before = torch.cat([b.param_flat.clone() for b in eng.reducer._buckets])
        eng.train_step(x, y)
        after = torch.cat([b.param_flat for b in eng.reducer._buckets])
        want = 1e-2 * min(norm, max_norm)
        got = float((after - before).double().norm())
        assert abs(got - want) <= 1e-3 * want, (got, want)
        assert float(eng.last_grad_norm) == norm
    assert _engine().setup().clipper is None


def test_engine_refuses_clipping_under_dgc():
    for kw in (dict(clip_grad_norm=1.0), dict(skip_nonfinite=True)):
        for dgc_kw in (dict(dgc=True),
                       dict(dgc=True, dgc_momentum_correction=True)):
            with pytest.raises(ValueError):
                _engine(**kw, **dgc_kw)
    with pytest.raises(ValueError):
        _engine(clip_grad_norm=-1.0)


def test_strategy_field_and_cli_flags():
    from edl_amd.train import fleet, train_distill, train_resnet

    assert fleet.DistributedStrategy().clip_grad_norm is None
    eng = fleet.distributed_engine(
        "mnist_mlp", fleet.DistributedStrategy(use_amp=False,
                                               clip_grad_norm=0.5),
        per_device_batch=8, num_classes=10, channels_last=False,
        use_hip_ops=False)
    assert eng.clip_grad_norm == 0.5
    assert isinstance(eng.clipper, GradClipper) and eng.clipper.max_norm == 0.5
    for mod in (train_resnet, train_distill):
        a = mod.parse_args([])
        assert (a.clip_grad_norm, a.skip_nonfinite) == (None, 0)
        a = mod.parse_args(["--clip_grad_norm", "2.5",
                            "--skip_nonfinite", "1"])
        assert (a.clip_grad_norm, a.skip_nonfinite) == (2.5, 1)


def test_train_simple_ctr_adam_clipped():
    env = dict(os.environ)
    env.update({"CUDA_VISIBLE_DEVICES": "", "PYTHONPATH": REPO})
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run(
        [sys.executable, "-m", "edl_amd.train.train_simple", "--model", "ctr",
         "--optimizer", "adam", "--lr", "1e-4", "--num_epochs", "1",
         "--steps_per_epoch", "5", "--clip_grad_norm", "0.1",
         "--skip_nonfinite", "1"],
        env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ctr epoch 0 loss=" in out.stdout + out.stderr


def test_two_rank_gloo_clips_the_averaged_gradient():
    """Different gradients per rank: both ranks end bit-equal, and match
    one process clipping the averaged gradient."""
    env = dict(os.environ)
    env.update({"EDL_REPO": REPO, "CUDA_VISIBLE_DEVICES": ""})
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29557", "--no-python", sys.executable,
         os.path.join(REPO, "tests", "_clip_gloo_worker.py")],
        env=env, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("CLIP_GLOO_OK") == 2, out.stdout[-3000:]
