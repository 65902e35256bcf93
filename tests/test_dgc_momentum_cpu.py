"""DGC with momentum correction, torch path: the selection rule, masking,
the sparsity schedule, re-bucketing, the engine's fp16 refusal, the
FusedSGD overrides, and a 2-rank gloo run of the engine.

The two tie cases use exact_inputs(70_001) (draw order g, u, v, p; the
counts below come from a plain sort, not from the code under test):
k=683 has count(a >= P) = 685 > k and count(a > P) = 682, so the tie
crosses the boundary and 682 are sent; k=n has P = 0 and sends the
69_996 non-zero values."""
import os
import subprocess
import sys

import pytest
import torch

from _dgc_momentum_common import (MU, WD, exact_inputs, payload_indices,
                                  ref_select)
from edl_amd.ops.dgc import dgc_compress, dgc_decode
from edl_amd.ops.sgd import FusedSGD
from edl_amd.train.bucketed_ddp import BucketedAllReducer
from edl_amd.train.dgc import DGCMomentum

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70_001


def _accumulated(g, u, v, p, mu, wd):
    u2 = mu * u + (g + wd * p if p is not None else g)
    return u2, v + u2


@pytest.mark.parametrize("k,nsel", [(683, 682), (701, 700), (N, 69_996)])
def test_rule_on_tied_inputs(k, nsel):
    g, u, v, p = exact_inputs(N)
    u_acc, v_acc = _accumulated(g, u, v, p, MU, WD)
    want = ref_select(v_acc, k)
    assert want.numel() == nsel  # the sort-based rule, cross-checked
    payload = dgc_compress(g, u, v, p, MU, WD, k)
    assert payload.shape == (2, k) and payload.dtype == torch.int32
    got = payload_indices(payload)
    assert got.numel() == nsel and torch.equal(got, want)
    assert int((payload[0] < 0).sum()) == k - nsel
    # the values are v at the sent indices, bit for bit
    order = torch.sort(payload[0], stable=True).indices[k - nsel:]
    assert torch.equal(payload[1][order].view(torch.float32), v_acc[want])
    # masking: u and v are zero exactly at the sent indices
    keep = torch.ones(N, dtype=torch.bool)
    keep[want] = False
    assert torch.equal(v[want], torch.zeros(nsel))
    assert torch.equal(u[want], torch.zeros(nsel))
    assert torch.equal(v[keep], v_acc[keep]) and torch.equal(u[keep], u_acc[keep])
    if k < N:
        assert float(v_acc[want].abs().min()) > float(v.abs().max())


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n,k", [(2_100_003, 2100), (70_001, 70), (1021, 10)])
def test_randn_selects_exactly_topk(n, k, seed):
    gen = torch.Generator().manual_seed(seed)
    g, u, v, p = (torch.randn(n, generator=gen) for _ in range(4))
    _, v_acc = _accumulated(g, u, v, p, 0.9, 1e-4)
    payload = dgc_compress(g, u, v, p, 0.9, 1e-4, k)
    got = payload_indices(payload)
    assert got.numel() == k
    # v_acc here is torch's own evaluation of the same expression
    want = torch.sort(torch.topk(v_acc.abs(), k).indices).values
    assert torch.equal(got, want)


def test_all_zero_sends_nothing():
    z = torch.zeros(257)
    u, v = z.clone(), z.clone()
    payload = dgc_compress(z.clone(), u, v, None, 0.9, 0.0, 5)
    assert torch.equal(payload[0], torch.full((5,), -1, dtype=torch.int32))
    assert torch.equal(payload[1], torch.zeros(5, dtype=torch.int32))
    out = torch.ones(257)
    dgc_decode(out, [payload, payload])
    assert torch.equal(out, z)


def test_non_finite_sorts_first():
    g, u, v, p = exact_inputs(1021)
    g[5] = float("inf")
    g[700] = float("nan")
    payload = dgc_compress(g, u, v, p, MU, WD, 2)
    assert payload_indices(payload).tolist() == [5, 700]
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(u).all())


def test_decode_rank_order_and_empty_slots():
    def pl(idx, vals):
        return torch.stack([torch.tensor(idx, dtype=torch.int32),
                            torch.tensor(vals).view(torch.int32)])

    pls = [pl([3, -1, 0], [1e8, 0.0, 1.0]), pl([-1, 3, 7], [0.0, 1.0, 2.0]),
           pl([3, 0, -1], [-1e8, 0.5, 0.0])]
    out = torch.full((9,), 5.0)
    dgc_decode(out, pls)
    want = torch.zeros(9)
    want[3] = (torch.tensor(1e8) + 1.0) - 1e8  # rank order: 0.0, not 1.0
    want[0] = 1.5
    want[7] = 2.0
    assert torch.equal(out, want)


def test_schedule_index_five_entries():
    m = torch.nn.Linear(4, 4)
    r = BucketedAllReducer(m.parameters(), bucket_cap_mb=1)
    sp = (0.75, 0.9375, 0.984375, 0.996, 0.999)
    d = DGCMomentum(r, None, 0.9, 0.0, rampup_begin_step=2, rampup_step=10,
                    sparsity=sp)
    assert [d.in_dgc_phase(s) for s in (1, 2, 3)] == [False, False, True]
    got = [d.sparsity_index(s) for s in range(3, 15)]
    assert got == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4]
    assert d.k_for(1000, 3) == 250 and d.k_for(1000, 5) == 62
    assert d.k_for(1000, 14) == 1 and d.k_for(10, 14) == 1
    # the default rampup_step=1: entry 0 for one step, then the last
    d1 = DGCMomentum(r, None, 0.9, 0.0, sparsity=sp)
    assert [d1.sparsity_index(s) for s in (1, 2, 3)] == [0, 4, 4]


def _per_param(d):
    out = {}
    for st in d._state:
        for p, (off, n) in zip(st["params"], st["offsets"]):
            out[id(p)] = (st["u"][off:off + n].clone(),
                          st["v"][off:off + n].clone())
    return out


def test_rebuild_keeps_per_parameter_state():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.Tanh(),
                            torch.nn.Linear(64, 32), torch.nn.Linear(32, 8))
    r = BucketedAllReducer(m.parameters(), bucket_cap_mb=0.01)
    opt = FusedSGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4,
                   reducer=r)
    d = DGCMomentum(r, opt, 0.9, 1e-4, sparsity=(0.9,))
    nb = len(r._buckets)
    assert nb > 1
    for _ in range(2):
        r.zero_grad()
        m(torch.randn(8, 64)).pow(2).mean().backward()
        assert d.step() is True
        opt.step(**d.opt_overrides())
    before = _per_param(d)
    assert any(bool(u.ne(0).any()) for u, _ in before.values())
    r.rebuild(1)
    assert len(r._buckets) == 1 != nb
    after = _per_param(d)
    assert before.keys() == after.keys()
    for key, (u, v) in before.items():
        assert torch.equal(after[key][0], u) and torch.equal(after[key][1], v)
    # and the next step runs on the new layout
    r.zero_grad()
    m(torch.randn(8, 64)).pow(2).mean().backward()
    d.step()
    assert d._state[0]["u"].numel() == r._buckets[0].buffer.numel()


def test_dense_phase_is_todays_step():
    """s <= rampup_begin_step: finalize + the optimizer's own momentum."""
    torch.manual_seed(0)
    m = torch.nn.Linear(8, 8)
    r = BucketedAllReducer(m.parameters(), bucket_cap_mb=1)
    opt = FusedSGD(m.parameters(), lr=0.1, reducer=r)
    d = DGCMomentum(r, opt, 0.9, 1e-4, rampup_begin_step=3)
    m(torch.randn(2, 8)).sum().backward()
    g0 = r._buckets[0].buffer.clone()
    assert d.step(global_step=3) is False and d.opt_overrides() == {}
    assert torch.equal(r._buckets[0].buffer, g0) and d._state is None
    assert d.step(global_step=4) is True
    assert d.opt_overrides() == {"momentum": 0.0, "weight_decay": 0.0}


def test_fp16_scaler_refused():
    from edl_amd.train.engine import TrainerEngine

    with pytest.raises(ValueError, match="loss"):
        TrainerEngine(model="mnist_mlp", dtype="fp16", dgc=True,
                      dgc_momentum_correction=True)
    # the old compressor keeps accepting it
    TrainerEngine(model="mnist_mlp", dtype="fp16", dgc=True)


def test_fused_sgd_overrides():
    """No overrides: the update is what it was (the torch-fallback math of
    the parent, written out here); with 0.0, 0.0 it is plain SGD."""
    torch.manual_seed(1)
    lr, mu, wd, scale = 0.05, 0.9, 1e-2, 0.5
    m = torch.nn.Linear(16, 8)
    r = BucketedAllReducer(m.parameters(), bucket_cap_mb=1)
    opt = FusedSGD(m.parameters(), lr=lr, momentum=mu, weight_decay=wd,
                   grad_scale=scale, reducer=r)
    p_ref = r._buckets[0].param_flat.clone()
    m_ref = torch.zeros_like(p_ref)
    for _ in range(2):
        r.zero_grad()
        m(torch.randn(4, 16)).pow(2).sum().backward()
        g = r._buckets[0].buffer.mul(scale).add(p_ref, alpha=wd)
        m_ref.mul_(mu).add_(g)
        p_ref.add_(m_ref, alpha=-lr)
        opt.step()
        assert torch.equal(r._buckets[0].param_flat, p_ref)
        assert torch.equal(opt._buckets[0]["m"], m_ref)
    r.zero_grad()
    m(torch.randn(4, 16)).pow(2).sum().backward()
    upd = lr * (r._buckets[0].buffer * scale)
    want = p_ref - upd
    opt.step(momentum=0.0, weight_decay=0.0)
    # two roundings (the product, the sum), each within 2^-24 of a term
    # no larger than |p| + |update|; one unit of margin
    tol = 3 * 2.0 ** -24 * (p_ref.abs() + upd.abs())
    assert bool(((r._buckets[0].param_flat - want).abs() <= tol).all())
    assert bool(upd.abs().max() > 1e-3)  # far above the tolerance
    assert opt.param_groups[0]["momentum"] == mu  # the group is untouched


def test_fleet_dgc_configs_reach_the_engine():
    from edl_amd.train import fleet

    s = fleet.DistributedStrategy(
        use_dgc=True, dgc_configs={"rampup_begin_step": 1, "rampup_step": 4,
                                   "sparsity": [0.5, 0.75]})
    eng = fleet.distributed_engine("mnist_mlp", strategy=s, dtype="fp32",
                                   use_hip_ops=False, checkpoint_dir=None)
    assert isinstance(eng.dgc, DGCMomentum)
    assert (eng.dgc.rampup_begin_step, eng.dgc.rampup_step,
            eng.dgc.sparsity) == (1, 4, (0.5, 0.75))


def test_trainer_cli_flags():
    from edl_amd.train.train_resnet import parse_args

    a = parse_args(["--use_dgc", "1", "--rampup_begin_step", "2",
                    "--rampup_step", "6", "--dgc_sparsity", "0.75,0.9375,0.999"])
    assert (a.use_dgc, a.rampup_begin_step, a.rampup_step) == (1, 2, 6)
    assert [float(x) for x in a.dgc_sparsity.split(",")] == [0.75, 0.9375, 0.999]


def test_engine_two_rank_gloo_matches_plain_sgd():
    """sparsity 0.0 sends every non-zero value every step, so u and v are
    masked to zero each step and the engine must equal plain SGD with
    weight decay on the rank-averaged gradients (3 steps, rtol 1e-5)."""
    env = dict(os.environ)
    env.update({"EDL_REPO": REPO, "CUDA_VISIBLE_DEVICES": ""})
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29547", "--no-python", sys.executable,
         os.path.join(REPO, "tests", "_dgc_momentum_gloo_worker.py")],
        env=env, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("DGC_GLOO_OK") == 2, out.stdout[-3000:]
