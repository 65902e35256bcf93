"""What FusedSGD, FusedAdam and FusedLARS inherit from ops/flat_optimizer.py:
the state survives a re-bucketing bit for bit, and state_buffers() hands
out the live buffers."""
import pytest
import torch
import torch.nn as nn

from edl_amd.ops.adam import FusedAdam
from edl_amd.ops.lars import FusedLARS
from edl_amd.ops.sgd import FusedSGD
from edl_amd.train.bucketed_ddp import BucketedAllReducer


def _bias(p):
    return p.ndim == 1


MAKE = {
    "sgd": lambda ps, r: FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-2,
                                  reducer=r),
    "adam": lambda ps, r: FusedAdam(ps, lr=1e-2, weight_decay=1e-2,
                                    no_decay=_bias, reducer=r),
    "lars": lambda ps, r: FusedLARS(ps, lr=0.1, lars_coeff=0.02, exclude=_bias,
                                    reducer=r),
}


def _stepped(kind, cap_mb=0.001):
    """A two-layer MLP (3856 bytes of params) under a 1048-byte bucket cap,
    after two steps -> (reducer, optimizer)."""
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(20, 30), nn.ReLU(), nn.Linear(30, 10))
    params = list(model.parameters())
    r = BucketedAllReducer(params, bucket_cap_mb=cap_mb)
    opt = MAKE[kind](params, r)
    assert len(r._buckets) >= 2
    for _ in range(2):
        opt.zero_grad()
        model(torch.randn(8, 20)).pow(2).mean().backward()
        opt.step()
    return r, opt


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return a.dtype == b.dtype and torch.equal(a, b)
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("kind", ["sgd", "adam", "lars"])
def test_state_dict_survives_rebuild_bit_for_bit(kind):
    r, opt = _stepped(kind)
    before = opt.state_dict()
    old = opt.state_buffers()
    assert any(bool(t.ne(0).any()) for t in old)
    nb = len(r._buckets)
    r.rebuild(25)
    assert len(r._buckets) == 1 != nb
    after = opt.state_dict()
    assert _same(before, after)
    new = opt.state_buffers()
    flats = [bk[name] for bk in opt._materialize()
             for name in ("m", "v") if name in bk]
    assert flats and all(any(t is f for t in new) for f in flats)
    old_ptrs = {t.data_ptr() for t in old if t.numel() > 1}
    assert not old_ptrs & {f.data_ptr() for f in flats}


def test_sgd_state_buffers_are_the_momentum_buffers():
    _, opt = _stepped("sgd")
    bufs = opt.state_buffers()
    ms = [bk["m"] for bk in opt._materialize()]
    assert len(bufs) == len(ms) >= 2
    assert all(a is b for a, b in zip(bufs, ms))
