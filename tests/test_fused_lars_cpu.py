"""FusedLARS on CPU (the torch twin of ops/lars.py): numerics against the
plain per-tensor LARS of _lars_common under its tolerance rule, the trust-1
branches, the state dict, elastic rebuild, the clip state, and the engine /
strategy / CLI plumbing, including a 2-rank gloo run."""
import copy
import os
import subprocess
import sys

import pytest
import torch

import _adam_common as A
import _lars_common as L
from edl_amd.ops.lars import FusedLARS
from edl_amd.ops.sgd import FusedSGD
from edl_amd.train.bucketed_ddp import BucketedAllReducer
from edl_amd.train.engine import TrainerEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fused(layout, offset=0, cap_mb=25, **kw):
    p0, grads, truth, ref = L.case_reference(layout, offset)
    params = L.make_params(layout, p0)
    r, opt = L.make_opt(params, layout, cap_mb, **kw)
    return params, r, opt, grads, truth, ref


def test_matches_truth_on_ragged_layout():
    layout = L.ragged_layout()
    params, _, opt, grads, truth, ref = _fused(layout)
    got = L.run_opt(params, layout, opt, grads)
    L.check(L.run_errors(got, truth), ref, "cpu ragged")
    assert float(truth[-1][1].abs().max()) > 0  # the velocities really moved
    assert bool((truth[-1][2] != 1).any())


def test_excluded_tensors_follow_plain_momentum_exactly():
    layout = L.ragged_layout()
    params, _, opt, grads, _, _ = _fused(layout)
    got = L.run_opt(params, layout, opt, grads)
    h = L.HYPER
    p0, _ = A.make_inputs(sum(L.RAGGED))
    lr = torch.tensor(h["lr"], dtype=torch.float32)
    for s, e, ex in L.spans(layout):
        if not ex:
            continue
        p, v = p0[s:e].float(), torch.zeros(e - s)
        for g in grads:
            v = v * h["momentum"] + (g[s:e].float() * L.GRAD_SCALE) * lr
            p = p - v
        assert torch.equal(got[-1][0][s:e], p)
        assert torch.equal(got[-1][1][s:e], v)
    k_ex = [k for k, (_, ex) in enumerate(layout) if ex]
    assert k_ex and bool((got[-1][2][k_ex] == 1).all())


def test_zero_p_and_zero_g_tensors_get_trust_one():
    # elements 0..2: p == 0; element 55: g == 0 (55 % 7 == 6), p != 0
    layout = [(3, False), (52, False), (1, False), (9, False)]
    params, _, opt, grads, truth, ref = _fused(layout)
    assert not bool(params[0].ne(0).any()) and bool(params[2].ne(0).all())
    assert all(float(g[55]) == 0.0 for g in grads)
    got = L.run_opt(params, layout, opt, grads[:1])
    tr = got[0][2]
    print("trust:", tr.tolist())
    assert float(tr[0]) == 1.0 and float(tr[2]) == 1.0
    assert float(tr[1]) != 1.0 and float(tr[3]) != 1.0
    L.check(L.run_errors(got, truth), ref, "cpu trust-1 branches")


def test_state_dict_roundtrip_and_sgd_does_not_take_it():
    layout = L.ragged_layout()
    params, _, opt, grads, _, _ = _fused(layout)
    L.run_opt(params, layout, opt, grads[:3])
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(len(layout)))
    assert sorted(sd["state"][0]) == ["velocity"]
    g0 = sd["param_groups"][0]
    assert {k: g0[k] for k in L.HYPER} == L.HYPER
    assert g0["exclude"] == [3, 7]

    # a fresh twin with other hyper-parameters takes all of it
    p2 = [torch.nn.Parameter(p.detach().clone()) for p in params]
    _, opt2 = L.make_opt(p2, layout, lr=0.5, lars_coeff=1.0, momentum=0.0)
    opt2.load_state_dict(copy.deepcopy(sd))
    assert {k: opt2.param_groups[0][k] for k in L.HYPER} == L.HYPER
    a = L.run_opt(params, layout, opt, grads[3:5])[-1]
    b = L.run_opt(p2, layout, opt2, grads[3:5])[-1]
    for x, y in zip(a, b):
        assert torch.equal(x, y)

    # FusedSGD must not mistake the LR-holding velocity for its momentum
    p3 = [torch.nn.Parameter(p.detach().clone()) for p in params]
    r3 = BucketedAllReducer(p3, bucket_cap_mb=25)
    sgd = FusedSGD(p3, lr=0.1, reducer=r3)
    sgd.load_state_dict(copy.deepcopy(sd))
    assert not any(bool(bk["m"].ne(0).any()) for bk in sgd._materialize())


def test_load_refuses_another_exclusion_set():
    layout = L.ragged_layout()
    params, _, opt, grads, _, _ = _fused(layout)
    L.run_opt(params, layout, opt, grads[:2])
    sd = opt.state_dict()
    other = L.ragged_layout({3})
    p2 = L.make_params(other, A.make_inputs(sum(L.RAGGED))[0])
    _, opt2 = L.make_opt(p2, other, lr=0.5)
    with pytest.raises(ValueError):
        opt2.load_state_dict(copy.deepcopy(sd))
    # nothing was loaded
    assert opt2.param_groups[0]["lr"] == 0.5
    assert not any(bool(v.ne(0).any()) for v in opt2.state_buffers())


def test_elastic_rebuild_carries_state_bit_for_bit():
    layout = L.ragged_layout()
    pa, _, oa, grads, _, _ = _fused(layout)
    pb, rb, ob, _, _, _ = _fused(layout)
    a = L.run_opt(pa, layout, oa, grads[:4])[-1]
    L.run_opt(pb, layout, ob, grads[:3])
    assert len(rb._buckets) == 1
    rb.rebuild(0.004)  # ~4 KB cap: the 20980 bytes split several ways
    assert len(rb._buckets) > 2
    assert len(ob._materialize()) == len(rb._buckets)
    b = L.run_opt(pb, layout, ob, grads[3:4])[-1]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_clip_state_skip_and_coef():
    layout = L.ragged_layout()
    # skip: p and v untouched, NaN gradients present
    params, _, opt, grads, _, _ = _fused(layout)
    L.run_opt(params, layout, opt, grads[:1])
    before = L.opt_state(params, opt)
    bad = grads[1].clone()
    bad[5] = float("nan")
    skip = torch.tensor([0.0, float("nan"), 1.0, 1.0])
    after = L.run_opt(params, layout, opt, [bad], clip_state=skip)[-1]
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    # coef: 0.5 on grad_scale 0.25 is bitwise grad_scale 0.125 without clip
    # (exact powers of two), in the gradient norm too
    pa, _, oa, _, _, _ = _fused(layout, grad_scale=0.25)
    pb, _, ob, _, _, _ = _fused(layout)
    half = torch.tensor([0.5, 3.0, 0.0, 0.0])
    a = L.run_opt(pa, layout, oa, grads[:2], clip_state=half)[-1]
    b = L.run_opt(pb, layout, ob, grads[:2])[-1]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # coef 1.0 is the null path
    pc, _, oc, _, _, _ = _fused(layout)
    one = torch.tensor([1.0, 3.0, 0.0, 0.0])
    c = L.run_opt(pc, layout, oc, grads[:2], clip_state=one)[-1]
    for x, y in zip(b, c):
        assert torch.equal(x, y)


def _engine(tmp_path=None, **kw):
    kw.setdefault("optimizer", "lars")
    kw.setdefault("base_lr", 0.1)
    return TrainerEngine(
        model="mnist_mlp", per_device_batch=8, num_classes=10,
        weight_decay=5e-4, label_smoothing=0.0, dtype="fp32",
        channels_last=False, use_hip_ops=False,
        checkpoint_dir=str(tmp_path / "ck") if tmp_path else None, **kw)


def test_engine_trains_checkpoints_and_resumes_lars(tmp_path):
    kw = dict(no_decay_1d=True, lars_coeff=0.02, lars_eps=1e-9,
              clip_grad_norm=5.0, skip_nonfinite=True)
    eng = _engine(tmp_path, **kw).setup()
    assert isinstance(eng.opt, FusedLARS)
    g0 = eng.opt.param_groups[0]
    assert (g0["lars_coeff"], g0["lars_weight_decay"], g0["epsilon"],
            g0["momentum"]) == (0.02, 5e-4, 1e-9, 0.9)
    n1d = [i for i, p in enumerate(eng.model.parameters()) if p.ndim <= 1]
    assert n1d and g0["exclude"] == n1d
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(8, 1, 28, 28, generator=gen)
    y = torch.randint(0, 10, (8,), generator=gen)
    losses = [eng.train_step(x, y).item() for _ in range(10)]
    print("losses:", losses)
    assert losses[-1] < losses[0], losses
    tr = eng.last_trust_ratios
    assert tr.shape == (len(list(eng.model.parameters())),)
    assert bool((tr[n1d] == 1).all()) and bool((tr != 1).any())
    # the momentum schedule: linear scaling, warmup and piecewise decay
    sgd = _engine(optimizer="momentum")
    for e, s in ((0, 0.0), (2, 0.5), (10, 0.0), (35, 0.0), (95, 0.25)):
        assert eng.scaled_lr(e, s) == sgd.scaled_lr(e, s)
    assert eng.scaled_lr(10) == pytest.approx(0.1 * 8 / 256)
    assert eng.scaled_lr(2) < eng.scaled_lr(10) > eng.scaled_lr(35)
    eng.save_checkpoint(0, blocking=True)
    eng.ckpt.wait()

    eng2 = _engine(tmp_path, **kw).setup()
    a, b = eng.opt.state_dict()["state"], eng2.opt.state_dict()["state"]
    assert len(a) == len(b) == len(list(eng.model.parameters()))
    for i in a:
        assert torch.equal(a[i]["velocity"], b[i]["velocity"])
        assert bool(a[i]["velocity"].ne(0).any())
    assert torch.equal(eng.train_step(x, y), eng2.train_step(x, y))
    for p, q in zip(eng.model.parameters(), eng2.model.parameters()):
        assert torch.equal(p, q)


def test_engine_refuses_lars_with_dgc():
    with pytest.raises(ValueError):
        _engine(dgc=True)
    with pytest.raises(ValueError):
        _engine(dgc=True, dgc_momentum_correction=True)


def test_distributed_strategy_maps_lars_configs(monkeypatch):
    from edl_amd.train import fleet

    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    st = fleet.DistributedStrategy(use_amp=False)
    assert st.lars is False and st.lars_configs == {}
    st = fleet.DistributedStrategy(
        use_amp=False, lars=True,
        lars_configs={"lars_coeff": 0.01, "lars_weight_decay": 1e-3,
                      "epsilon": 1e-8,
                      "exclude_from_weight_decay": ["bias"]})
    eng = fleet.distributed_engine(
        "mnist_mlp", st, per_device_batch=8, num_classes=10,
        channels_last=False, use_hip_ops=False)
    assert isinstance(eng.opt, FusedLARS)
    g0 = eng.opt.param_groups[0]
    assert (g0["lars_coeff"], g0["lars_weight_decay"], g0["epsilon"]) == (
        0.01, 1e-3, 1e-8)
    names = [n for n, _ in eng.model.named_parameters()]
    want = [i for i, n in enumerate(names) if "bias" in n]
    assert want and len(want) < len(names) and g0["exclude"] == want
    bad = fleet.DistributedStrategy(lars=True, lars_configs={"coeff": 1.0})
    with pytest.raises(ValueError, match="coeff"):
        fleet.distributed_engine("mnist_mlp", bad)


def test_cli_flags():
    from edl_amd.train import train_distill, train_resnet

    for mod in (train_resnet, train_distill):
        a = mod.parse_args([])
        assert (a.optimizer, a.lars_coeff, a.lars_eps) == (
            "momentum", 0.001, 0.0)
        a = mod.parse_args(["--optimizer", "lars", "--lars_coeff", "0.02",
                            "--lars_eps", "1e-9"])
        assert (a.optimizer, a.lars_coeff, a.lars_eps) == ("lars", 0.02, 1e-9)


def test_train_simple_lars():
    """train_simple --model ctr --optimizer lars runs (single process)."""
    env = dict(os.environ)
    env.update({"CUDA_VISIBLE_DEVICES": "", "PYTHONPATH": REPO})
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run(
        [sys.executable, "-m", "edl_amd.train.train_simple", "--model", "ctr",
         "--optimizer", "lars", "--lars_coeff", "0.02", "--lr", "1e-2",
         "--num_epochs", "1", "--steps_per_epoch", "5"],
        env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ctr epoch 0 loss=" in out.stdout + out.stderr


def test_two_rank_gloo_identical_bits(tmp_path):
    """Ranks resume from different local checkpoints; setup() must leave
    rank 0's velocities on both, and 3 clipped LARS steps later params,
    velocities and trust ratios agree bit for bit."""
    env = dict(os.environ)
    env.update({"EDL_REPO": REPO, "CUDA_VISIBLE_DEVICES": ""})
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29557", "--no-python", sys.executable,
         os.path.join(REPO, "tests", "_lars_gloo_worker.py"), str(tmp_path)],
        env=env, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("LARS_GLOO_OK") == 2, out.stdout[-3000:]
