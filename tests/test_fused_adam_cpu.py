"""FusedAdam / FusedAdamW on CPU (the torch path of ops/adam.py): numerics
against torch.optim under the tolerance rule of _adam_common, state-dict
interchange with torch, elastic rebuild, per-param decay exemption, and
the engine / CLI plumbing, including a 2-rank gloo state sync."""
import copy
import os
import subprocess
import sys

import pytest
import torch

import _adam_common as C
from edl_amd.ops.adam import FusedAdam, FusedAdamW
from edl_amd.train.bucketed_ddp import BucketedAllReducer
from edl_amd.train.engine import TrainerEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(dtype=torch.float32):
    """The small two-layer model, its params set from _adam_common's
    index-defined values (in parameters() order)."""
    m = torch.nn.Sequential(torch.nn.Linear(10, 64), torch.nn.ReLU(),
                            torch.nn.Linear(64, 4)).to(dtype)
    n = sum(p.numel() for p in m.parameters())
    p0, grads = C.make_inputs(n)
    off = 0
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p0[off:off + p.numel()].view_as(p))
            off += p.numel()
    return m, grads


def _set_grads(model, flat, scale=1.0):
    off = 0
    for p in model.parameters():
        g = (flat[off:off + p.numel()] * scale).view_as(p).to(p.dtype)
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)
        off += p.numel()


def _flat_state(model, opt_state):
    """(p, m, v) flat in parameters() order; opt_state: index -> entry."""
    ps = list(model.parameters())
    return (torch.cat([p.detach().reshape(-1) for p in ps]),
            torch.cat([opt_state[i]["exp_avg"].reshape(-1)
                       for i in range(len(ps))]),
            torch.cat([opt_state[i]["exp_avg_sq"].reshape(-1)
                       for i in range(len(ps))]))


def _fused(model, mode, cap_mb=25, **kw):
    r = BucketedAllReducer(model.parameters(), bucket_cap_mb=cap_mb)
    cls = FusedAdam if mode == "l2" else FusedAdamW
    kw.setdefault("weight_decay", C.WD[mode])
    kw.setdefault("grad_scale", C.GRAD_SCALE)
    return r, cls(model.parameters(), reducer=r, **dict(C.HYPER, **kw))


def _torch_opt(model, mode, groups=None, **kw):
    cls = torch.optim.Adam if mode == "l2" else torch.optim.AdamW
    kw.setdefault("weight_decay", C.WD[mode])
    return cls(groups or model.parameters(), foreach=False,
               **dict(C.HYPER, **kw))


def _torch_state(model, opt):
    return {i: opt.state[p] for i, p in enumerate(model.parameters())}


def _run_torch(model, opt, grads):
    out = []
    for g in grads:
        _set_grads(model, g, C.GRAD_SCALE)
        opt.step()
        out.append(_flat_state(model, _torch_state(model, opt)))
    return out


def _run_fused(model, opt, grads):
    out = []
    for g in grads:
        _set_grads(model, g)
        opt.step()
        out.append(_flat_state(model, opt.state_dict()["state"]))
    return out


@pytest.mark.parametrize("mode", ["l2", "decoupled"])
def test_matches_torch_over_six_steps(mode):
    m64, grads = _model(torch.float64)
    truth = _run_torch(m64, _torch_opt(m64, mode), grads)
    m32, _ = _model()
    ref = C.run_errors(_run_torch(m32, _torch_opt(m32, mode), grads), truth)
    mf, _ = _model()
    _, opt = _fused(mf, mode)
    got = C.run_errors(_run_fused(mf, opt, grads), truth)
    C.check(got, ref, "cpu two-layer " + mode)
    assert opt.step_count == C.STEPS
    assert float(truth[-1][1].abs().max()) > 0  # the moments really moved


def test_grad_scale_folding_is_exact():
    ma, grads = _model()
    mb, _ = _model()
    _, oa = _fused(ma, "l2", grad_scale=1.0)
    _, ob = _fused(mb, "l2", grad_scale=0.5)
    a = _run_fused(ma, oa, grads)[-1]
    b = _run_fused(mb, ob, [g * 2 for g in grads])[-1]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_state_dict_loads_into_torch_adam_and_back():
    hyper = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6)
    mf, grads = _model()
    _, opt = _fused(mf, "l2", **hyper)
    _run_fused(mf, opt, grads[:3])
    sd = opt.state_dict()
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert float(sd["state"][0]["step"]) == 3.0
    g0 = sd["param_groups"][0]
    assert (g0["lr"], tuple(g0["betas"]), g0["eps"], g0["amsgrad"]) == (
        3e-3, (0.8, 0.99), 1e-6, False)

    # fused -> torch (fp32 and the fp64 truth), then 2 more steps each
    m32, m64 = copy.deepcopy(mf), copy.deepcopy(mf).double()
    o32, o64 = _torch_opt(m32, "l2"), _torch_opt(m64, "l2")
    o32.load_state_dict(copy.deepcopy(sd))
    o64.load_state_dict(copy.deepcopy(sd))
    tg = o32.param_groups[0]
    assert (tg["lr"], tuple(tg["betas"]), tg["eps"]) == (3e-3, (0.8, 0.99), 1e-6)
    assert all(float(o32.state[p]["step"]) == 3.0 for p in m32.parameters())
    truth = _run_torch(m64, o64, grads[3:5])
    ref = C.run_errors(_run_torch(m32, o32, grads[3:5]), truth)
    got = C.run_errors(_run_fused(mf, opt, grads[3:5]), truth)
    C.check(got, ref, "cpu fused->torch continue")
    assert float(o32.state[next(m32.parameters())]["step"]) == 5.0

    # torch -> fused: a fresh FusedAdam with OTHER hyper-parameters takes
    # torch's state, lr, betas, eps and step
    tsd = o32.state_dict()
    mf2 = copy.deepcopy(m32)
    _, opt2 = _fused(mf2, "l2")
    opt2.load_state_dict(copy.deepcopy(tsd))
    g2 = opt2.param_groups[0]
    assert (g2["lr"], g2["betas"], g2["eps"]) == (3e-3, (0.8, 0.99), 1e-6)
    assert opt2.step_count == 5
    for a, b in zip(_flat_state(mf2, opt2.state_dict()["state"]),
                    _flat_state(m32, _torch_state(m32, o32))):
        assert torch.equal(a, b)
    m64b = copy.deepcopy(m32).double()
    o64b = _torch_opt(m64b, "l2")
    o64b.load_state_dict(copy.deepcopy(tsd))
    truth = _run_torch(m64b, o64b, grads[4:6])
    ref = C.run_errors(_run_torch(m32, o32, grads[4:6]), truth)
    got = C.run_errors(_run_fused(mf2, opt2, grads[4:6]), truth)
    C.check(got, ref, "cpu torch->fused continue")
    assert opt2.step_count == 7


def test_load_refuses_another_decay_mode():
    """`decoupled` and the no_decay set are construction-time choices: a
    state dict recording other ones is refused, nothing is loaded."""
    ma, grads = _model()
    _, ow = _fused(ma, "decoupled", no_decay=lambda p: p.ndim <= 1)
    _run_fused(ma, ow, grads[:2])
    sd = ow.state_dict()
    for mode, kw in (("l2", dict(no_decay=lambda p: p.ndim <= 1)),
                     ("decoupled", {})):
        mb, _ = _model()
        _, ob = _fused(mb, mode, **kw)
        with pytest.raises(ValueError):
            ob.load_state_dict(copy.deepcopy(sd))
        assert ob.step_count == 0
        assert not bool(ob._materialize()[0]["m"].ne(0).any())
    mc, _ = _model()
    _, oc = _fused(mc, "decoupled", no_decay=lambda p: p.ndim <= 1)
    oc.load_state_dict(copy.deepcopy(sd))
    assert oc.step_count == 2


def test_elastic_rebuild_carries_state():
    ma, grads = _model()
    mb, _ = _model()
    _, oa = _fused(ma, "decoupled", no_decay=lambda p: p.ndim <= 1)
    rb, ob = _fused(mb, "decoupled", no_decay=lambda p: p.ndim <= 1)
    a = _run_fused(ma, oa, grads[:5])[-1]
    _run_fused(mb, ob, grads[:3])
    assert len(rb._buckets) == 1
    rb.rebuild(0.001)  # 1048-byte cap: the 3856 bytes split three ways
    assert len(rb._buckets) == 3
    b = _run_fused(mb, ob, grads[3:5])[-1]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert oa.step_count == ob.step_count == 5


def test_no_decay_predicate_matches_two_param_groups():
    def groups(model):
        ps = list(model.parameters())
        return [{"params": [p for p in ps if p.ndim > 1]},
                {"params": [p for p in ps if p.ndim <= 1],
                 "weight_decay": 0.0}]

    m64, grads = _model(torch.float64)
    truth = _run_torch(m64, _torch_opt(m64, "decoupled", groups(m64)), grads)
    m32, _ = _model()
    ref = C.run_errors(
        _run_torch(m32, _torch_opt(m32, "decoupled", groups(m32)), grads),
        truth)
    mf, _ = _model()
    _, opt = _fused(mf, "decoupled", no_decay=lambda p: p.ndim <= 1)
    assert len(opt._materialize()[0]["segs"]) == 4  # b2, w2, b1, w1
    got = C.run_errors(_run_fused(mf, opt, grads), truth)
    C.check(got, ref, "cpu no_decay")
    # an iterable of params selects the same set, and it matters
    mi, _ = _model()
    _, opt_i = _fused(mi, "decoupled",
                      no_decay=[p for p in mi.parameters() if p.ndim <= 1])
    assert opt_i.state_dict()["param_groups"][0]["no_decay"] == [1, 3]
    for a, b in zip(_run_fused(mi, opt_i, grads)[-1],
                    _flat_state(mf, opt.state_dict()["state"])):
        assert torch.equal(a, b)
    mu, _ = _model()
    _, opt_u = _fused(mu, "decoupled")
    assert opt_u._materialize()[0]["segs"] == [[964, C.WD["decoupled"]]]
    assert not torch.equal(_run_fused(mu, opt_u, grads)[-1][0],
                           _flat_state(mf, opt.state_dict()["state"])[0])


def _engine(tmp_path=None, **kw):
    kw.setdefault("optimizer", "adamw")
    return TrainerEngine(
        model="mnist_mlp", per_device_batch=8, num_classes=10, base_lr=1e-3,
        weight_decay=1e-2, label_smoothing=0.0, dtype="fp32",
        channels_last=False, use_hip_ops=False,
        checkpoint_dir=str(tmp_path / "ck") if tmp_path else None, **kw)


def test_engine_trains_and_resumes_adamw(tmp_path):
    eng = _engine(tmp_path, no_decay_1d=True).setup()
    assert isinstance(eng.opt, FusedAdam)
    assert eng.opt.param_groups[0]["decoupled"] is True
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(8, 1, 28, 28, generator=gen)
    y = torch.randint(0, 10, (8,), generator=gen)
    losses = [eng.train_step(x, y).item() for _ in range(10)]
    assert losses[-1] < losses[0], losses
    assert eng.opt.step_count == 10
    # constant LR: no linear scaling, no piecewise decay, no warmup
    assert {eng.scaled_lr(e, s) for e in (0, 3, 40, 95)
            for s in (0.0, 0.5)} == {1e-3}
    eng.save_checkpoint(0, blocking=True)
    eng.ckpt.wait()

    eng2 = _engine(tmp_path, no_decay_1d=True).setup()
    assert eng2.opt.step_count == 10
    a, b = eng.opt.state_dict()["state"], eng2.opt.state_dict()["state"]
    assert len(a) == len(b) == len(list(eng.model.parameters()))
    for i in a:
        assert torch.equal(a[i]["exp_avg"], b[i]["exp_avg"])
        assert torch.equal(a[i]["exp_avg_sq"], b[i]["exp_avg_sq"])
        assert bool(a[i]["exp_avg_sq"].ne(0).any())
    # both continue identically
    assert torch.equal(eng.train_step(x, y), eng2.train_step(x, y))
    for p, q in zip(eng.model.parameters(), eng2.model.parameters()):
        assert torch.equal(p, q)


def test_engine_optimizer_selection():
    from edl_amd.ops.sgd import FusedSGD

    with pytest.raises(ValueError):
        _engine(optimizer="adam", dgc=True)
    with pytest.raises(ValueError):
        _engine(optimizer="rmsprop")
    eng = _engine(optimizer="adam", betas=(0.8, 0.99), eps=1e-6).setup()
    g0 = eng.opt.param_groups[0]
    assert (g0["decoupled"], g0["betas"], g0["eps"], g0["no_decay"]) == (
        False, (0.8, 0.99), 1e-6, [])
    default = TrainerEngine(
        model="mnist_mlp", per_device_batch=8, num_classes=10, dtype="fp32",
        channels_last=False, use_hip_ops=False).setup()
    assert isinstance(default.opt, FusedSGD)
    assert default.optimizer == "momentum"
    # the momentum engine keeps the linear-scaling piecewise schedule
    assert default.scaled_lr(35) != default.scaled_lr(0)


def test_cli_flags():
    from edl_amd.train import train_distill, train_resnet

    for mod in (train_resnet, train_distill):
        a = mod.parse_args([])
        assert (a.optimizer, a.beta1, a.beta2, a.epsilon, a.no_decay_1d) == (
            "momentum", 0.9, 0.999, 1e-8, 0)
        a = mod.parse_args(["--optimizer", "adamw", "--beta1", "0.8",
                            "--beta2", "0.99", "--epsilon", "1e-6",
                            "--no_decay_1d", "1"])
        assert (a.optimizer, a.beta1, a.beta2, a.epsilon, a.no_decay_1d) == (
            "adamw", 0.8, 0.99, 1e-6, 1)


def test_train_simple_ctr_adam():
    """train_simple --model ctr --optimizer adam runs (single process)."""
    env = dict(os.environ)
    env.update({"CUDA_VISIBLE_DEVICES": "", "PYTHONPATH": REPO})
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run(
        [sys.executable, "-m", "edl_amd.train.train_simple", "--model", "ctr",
         "--optimizer", "adam", "--lr", "1e-4", "--num_epochs", "1",
         "--steps_per_epoch", "5"],
        env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ctr epoch 0 loss=" in out.stdout + out.stderr


def test_train_simple_ctr_adam_under_edlrun(coord_server, tmp_path):
    """The issue's command line under the real launcher, 2 agents on gloo."""
    from test_train_scripts import run_edlrun

    run_edlrun(
        coord_server, tmp_path,
        ["-m", "edl_amd.train.train_simple", "--model", "ctr",
         "--optimizer", "adam", "--lr", "1e-4", "--num_epochs", "1",
         "--steps_per_epoch", "20", "--checkpoint", str(tmp_path / "ck")])
    assert (tmp_path / "ck" / "checkpoint.0").is_dir()


def test_two_rank_gloo_syncs_adam_state(tmp_path):
    """Ranks resume from different local checkpoints; setup() must leave
    rank 0's m, v and step on both, and 3 steps later the params agree."""
    env = dict(os.environ)
    env.update({"EDL_REPO": REPO, "CUDA_VISIBLE_DEVICES": ""})
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29553", "--no-python", sys.executable,
         os.path.join(REPO, "tests", "_adam_gloo_worker.py"), str(tmp_path)],
        env=env, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("ADAM_GLOO_OK") == 2, out.stdout[-3000:]
